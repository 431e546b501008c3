"""Cost of starting a keyframe's point seeds on the device from its FAST corners (plsvo_seeds_keyframe_detect) beside the
host path of the same tree.  Needs an MI355X; prints one JSON object and writes it to --out.

  Protocol of tools/bench_seedlist.py: one session, --streams streams, 640 x 480 textured pyramid slots, --reps + 1 consecutive steps per
  load with the first untimed, median (min - max) of the others, the C entry points alone on prepared ctypes arrays.  Every stream holds
  200 point + 80 line seeds in two keyframes; one plsvo_seeds_update is run and fetched before the steps, so that the last update's
  matches are there to mark cells (PLSVO_SEED_OCC_UPDATED; no selection is staged, so PLSVO_SEED_OCC_SELECTED is not part of either
  side).  Loads (--loads): 1 in 1, 1 in 4 and 1 in 16 streams active.
   resident  plsvo_seeds_keyframe_detect -> plsvo_seeds_keyframe_fetch on the host clock (enqueue, the three launches, the one wait, the
             reports' copy)
   host      what a caller does today: plsvo_seeds_fetch_rows (the whole shadow-row section), the grid from the rows (NumPy, vectorised
             over the batch), plsvo_hip_detect_fast with that grid on one slot per active stream (upload of the grid, the two launches,
             download of counts and corners), the bearings (NumPy, vectorised), plsvo_seeds_keyframe of the seeds.  Every stream's
             keyframe sits in a pyramid slot of its own on BOTH sides (copies of sixteen textures): the resident side reads them
             through its slot table, the host entry point as a slot range.  The event records of plsvo_seeds_keyframe are packed once, from the first step's corners
             (the images and the rows do not change between the steps): the binding's packing is on neither side.
  The point rows are reserved for all steps' seeds (cells per step), which the fetch of the rows on the host side pays for as well:
  that call's share is reported apart (of_it_fetch_rows_ms, without_fetch_rows_ms), and the claim is checked without it too.
  --resident-only runs the resident side alone (for a kernel trace in a run of its own).

usage: python tools/bench_seedstart.py [--reps 7] [--streams 4096] [--loads "1;4;16"] [--resident-only] [--out profiles/seedstart_bench.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_candidates as B   # noqa: E402
import bench_insert as BI      # noqa: E402

W, H, CELL = 640, 480, 25
CAM = (420.0, 415.0, 319.5, 239.5, W, H)
COLS, ROWS = -(-W // CELL), -(-H // CELL)
CELLS = COLS * ROWS
N_SP, N_SS = 200, 80
IDENT = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
T_CUR = [0.0, 0.0, 0.0, 1.0, 0.05, 0.02, 0.0]
f32 = np.float32


def make_seeds(rng):
    def obs(k):
        px = np.stack([rng.uniform(20, W - 20, k), rng.uniform(20, H - 20, k)], 1)
        f = np.stack([(px[:, 0] - CAM[2]) / CAM[0], (px[:, 1] - CAM[3]) / CAM[1], np.ones(k)], 1)
        return px, f / np.linalg.norm(f, axis=1, keepdims=True)
    zr = f32(1.0 / 2.0)
    par = lambda k: dict(a=np.full(k, 10, f32), b=np.full(k, 10, f32), mu=np.full(k, 1.0 / 4.0, f32), z_range=np.full(k, zr, f32), sigma2=np.full(k, zr * zr / f32(36), f32))
    px, f = obs(N_SP)
    p = par(N_SP)
    d = dict(batch_counter=0, pt_ref_kf=rng.integers(0, 2, N_SP), pt_batch_id=np.zeros(N_SP, np.int32), pt_px=px, pt_f=f, pt_level=rng.integers(0, 3, N_SP),
             pt_type=np.zeros(N_SP, np.uint8), pt_grad=np.tile([1.0, 0.0], (N_SP, 1)), pt_a=p["a"], pt_b=p["b"], pt_mu=p["mu"], pt_z_range=p["z_range"], pt_sigma2=p["sigma2"])
    (spx, sf), (epx, ef) = obs(N_SS), obs(N_SS)
    mid = sf + ef
    q = par(N_SS)
    d.update(seg_ref_kf=rng.integers(0, 2, N_SS), seg_batch_id=np.zeros(N_SS, np.int32), seg_px=(spx + epx) / 2, seg_f=mid / np.linalg.norm(mid, axis=1, keepdims=True), seg_sf=sf,
             seg_ef=ef, seg_spx=spx, seg_epx=epx, seg_level=rng.integers(0, 3, N_SS), seg_a=q["a"], seg_b=q["b"], seg_mu_s=q["mu"], seg_mu_e=q["mu"], seg_z_range_s=q["z_range"],
             seg_z_range_e=q["z_range"], seg_sigma2_s=q["sigma2"], seg_sigma2_e=q["sigma2"])
    return d


def empty_map(P, kf1_slot):
    z2, z3, zi = np.zeros((0, 2)), np.zeros((0, 3)), np.zeros(0, np.int32)
    return P.abi.CandidateMapJob(kf_T=[IDENT, IDENT], kf_slot=[0, kf1_slot], kf_pt_off=np.zeros(3, np.int32), kf_pt_lm=zi, kf_seg_off=np.zeros(3, np.int32), kf_seg_lm=zi,
                                 pt_pos=z3, pt_type=zi, pt_obs_off=np.zeros(1, np.int32), pt_obs_kf=zi, pt_obs_px=z2, pt_obs_f=z3, pt_obs_level=zi, pt_obs_type=np.zeros(0, np.uint8),
                                 pt_obs_grad=z2, seg_spos=z3, seg_epos=z3, seg_type=zi, seg_obs_off=np.zeros(1, np.int32), seg_obs_kf=zi, seg_obs_spx=z2, seg_obs_epx=z2,
                                 seg_obs_sf=z3, seg_obs_ef=z3, seg_obs_level=zi, pt_cand=zi, seg_cand=zi)


def stage(P, ctx, n, seed_pool, steps):
    """the tables, the lists with room for every step's seeds, and one fetched update whose matches mark cells"""
    ctx.candidates_reserve()
    ctx.candidates_reserve_landmarks(extra_pt=N_SP, extra_seg=N_SS)
    ctx.candidates_stage([empty_map(P, 3 + i) for i in range(n)], CAM, 30, 40, 8, 3, 10)   # stream i's second keyframe: a slot of its own
    ctx.seeds_reserve(extra_pt=steps * CELLS, extra_seg=0)
    ctx.seeds_stage([seed_pool[i % len(seed_pool)] for i in range(n)], CAM, max_n_kfs=1 << 30)
    ctx.seeds_update([dict(cur_slot=2, T_f_w=T_CUR)] * n)
    rep = ctx.seeds_update_fetch()
    return {"pt": np.sum([r["pt"] for r in rep], 0).tolist()}


def events_array(P, n, every):
    arr = (P.abi.SeedKfDetect * n)()
    for i, a in enumerate(arr):
        a.removed_kf = -1
        if i % every == 0:
            a.active, a.new_kf, a.occ_sources, a.depth_mean, a.depth_min = 1, 1, P.abi.SEED_OCC_UPDATED, 4.0, 2.0
    return arr


def resident_leg(P, ctx, n, every, steps, seed_pool):
    hist = stage(P, ctx, n, seed_pool, steps)
    arr, outs, pr = events_array(P, n, every), (P.abi.SeedKfReport * n)(), P.abi.detect_params(CELL, 3, 20, 20.0)
    ts, kern = [], []
    ctx.set_profiling(True)
    for k in range(steps):
        ctx.synchronize()
        ctx.reset_profiling()
        t0 = time.perf_counter()
        rc = ctx.L.plsvo_seeds_keyframe_detect(ctx.h, n, C.byref(pr), arr)
        rc2 = ctx.L.plsvo_seeds_keyframe_fetch(ctx.h, n, outs)
        ts.append(time.perf_counter() - t0)
        assert rc == 0 and rc2 == 0, (rc, rc2)
        kern.append(ctx.kernel_time(P.abi.K_NEWCAND)[0])
        assert not any(outs[i].no_room for i in range(0, n, every))
    ctx.set_profiling(False)
    new = [outs[i].n_new_pt for i in range(0, n, every)]
    return ts, kern, dict(update_status_counts=hist, new_seeds_per_active_stream=dict(min=int(min(new)), max=int(max(new)), mean=round(float(np.mean(new)), 1)),
                          occupied_cells_mean=round(float(np.mean([outs[i].n_occupied for i in range(0, n, every)])), 1))


def host_leg(P, ctx, n, every, steps, seed_pool):
    stage(P, ctx, n, seed_pool, steps)
    act = list(range(0, n, every))
    na = len(act)
    cap = ctx.seeds_capacity()[0]["pt"]
    # fetch_rows' buffers: one block for all streams, so that the grid below is vectorised (status and px_cur are all the grid needs)
    status, px = np.zeros((n, cap), np.int32), np.zeros((n, cap, 2))
    rows = (P.abi.SeedRows * n)()
    for i, r in enumerate(rows):
        r.pt_status, r.pt_px_cur = status[i].ctypes.data_as(P.abi.c_i32_p), px[i].ctypes.data_as(P.abi.c_double_p)
    occ, corners, counts = np.zeros((na, CELLS), np.uint8), np.zeros((na, CELLS), P.abi.CORNER_DTYPE), np.zeros(na, np.int32)
    pr = P.abi.detect_params(CELL, 3, 20, 20.0)
    ev, keep, ts, t_rows = None, None, [], []
    for k in range(steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        rc = ctx.L.plsvo_seeds_fetch_rows(ctx.h, n, rows)
        assert rc == 0, rc
        t_rows.append(time.perf_counter() - t0)
        n_rows = np.array([rows[i].n_pt for i in act])
        st, p = status[act], px[act]
        mark = (np.arange(cap)[None] < n_rows[:, None]) & ((st == 2) | (st == 3) | (st == 4)) & (p[..., 0] >= 0) & (p[..., 0] < W) & (p[..., 1] >= 0) & (p[..., 1] < H)
        occ[:] = 0
        si, ri = np.nonzero(mark)
        occ[si, (p[si, ri, 1] / CELL).astype(np.int64) * COLS + (p[si, ri, 0] / CELL).astype(np.int64)] = 1
        rc = ctx.L.plsvo_hip_detect_fast(ctx.h, 3, na, C.byref(pr), occ.ctypes.data_as(P.abi.c_u8_p), corners.ctypes.data_as(C.POINTER(P.abi.Corner)), counts.ctypes.data_as(P.abi.c_i32_p))
        assert rc == 0, rc
        valid = np.arange(CELLS)[None] < counts[:, None]
        cpx = np.stack([corners["x"][valid], corners["y"][valid]], 1).astype(np.float64)
        x, y = (cpx[:, 0] - CAM[2]) / CAM[0], (cpx[:, 1] - CAM[3]) / CAM[1]
        nrm = np.sqrt((x * x + y * y) + 1.0)
        f = np.stack([x / nrm, y / nrm, 1.0 / nrm], 1)
        lvl, typ, grad = corners["level"][valid].astype(np.int32), np.zeros(len(cpx), np.uint8), np.tile([1.0, 0.0], (len(cpx), 1))
        if ev is None:                                  # (packed once: the corners are the same at every step)
            ev, keep, at = (P.abi.SeedKf * n)(), (cpx, f, lvl, typ, grad), 0
            for a in ev:
                a.removed_kf = -1
            for j, i in enumerate(act):
                a, c = ev[i], int(counts[j])
                a.new_kf, a.n_pt, a.depth_mean, a.depth_min = 1, c, 4.0, 2.0
                a.pt_px, a.pt_f, a.pt_grad = (v[at:].ctypes.data_as(P.abi.c_double_p) for v in (cpx, f, grad))
                a.pt_level, a.pt_type = lvl[at:].ctypes.data_as(P.abi.c_i32_p), typ[at:].ctypes.data_as(P.abi.c_u8_p)
                at += c
        rc = ctx.L.plsvo_seeds_keyframe(ctx.h, n, ev)
        assert rc == 0, rc
        ctx.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts, dict(new_seeds_per_active_stream=dict(min=int(counts.min()), max=int(counts.max()), mean=round(float(counts.mean()), 1)),
                    of_it_fetch_rows_ms=BI.stats(t_rows[1:], 1e3, 3), without_fetch_rows_ms=BI.stats([a - b for a, b in zip(ts[1:], t_rows[1:])], 1e3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--loads", default="1;4;16", help="1 in N streams active; several loads separated by ;")
    ap.add_argument("--resident-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    P = importlib.import_module("pl-svo_amd")
    emulated = hasattr(P.capi.lib(), "plsvo_emu_build")   # a dry run of the tool's own code on the host emulation build: its figures mean nothing
    if not torch.cuda.is_available() and not emulated:
        raise SystemExit("bench_seedstart.py: no GPU (a timing needs the MI355X)")
    n, steps = args.streams, args.reps + 1
    res = {"what": f"tools/bench_seedstart.py: plsvo_seeds_keyframe_detect -> plsvo_seeds_keyframe_fetch beside the host path of the same tree; {W} x {H} textured slots, cell {CELL} "
                   f"({CELLS} cells), {N_SP} + {N_SS} seeds per stream beforehand, PLSVO_SEED_OCC_UPDATED",
           "device": "host emulation (dry run)" if emulated else torch.cuda.get_device_name(0), "reps": args.reps, "streams": n, "loads": []}
    rng = np.random.default_rng(2027)
    seed_pool = [make_seeds(rng) for _ in range(64)]
    ctx = P.capi.Context(0)
    try:
        n_host = n                                    # one slot per stream: the resident side's keyframes and the host side's slot range
        ctx.config_pyramids(3 + n_host, W, H, 3)
        tex = min(16, 3 + n_host)
        for slot in range(tex):
            ctx.build_pyramid(slot, B._texture(rng, W, H), 0)
        have = tex
        while have < 3 + n_host:                        # the streams' keyframe slots: copies of the same textures
            k = min(have - 3, 3 + n_host - have)
            ctx.copy_slots(have, 3, k)
            have += k
        for every in [int(s) for s in args.loads.split(";") if s]:
            r_t, r_k, info = resident_leg(P, ctx, n, every, steps, seed_pool)
            leg = {"active": f"1 in {every}", "active_streams": len(range(0, n, every)), "steps": steps, "resident_call_and_fetch_ms": BI.stats(r_t[1:], 1e3, 3),
                   "resident_launches_ms_by_event_pair": BI.stats(r_k[1:], 1.0, 4), "resident": info}
            if not args.resident_only:
                h_t, h_info = host_leg(P, ctx, n, every, steps, seed_pool)
                leg.update(host_path_ms=BI.stats(h_t[1:], 1e3, 3), host=h_info, resident_median_below_host_minimum=bool(np.median(r_t[1:]) < min(h_t[1:])),
                           resident_median_below_host_minimum_without_fetch_rows=bool(1e3 * np.median(r_t[1:]) < h_info["without_fetch_rows_ms"]["min"]))
            res["loads"].append(leg)
    finally:
        ctx.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
