"""Everything the pose optimiser reports on one small mixed batch, per launch shape, into ONE .npz with a fixed byte layout -- for holding
a build of the library to another bit for bit (the launch shapes sum in different orders, so no test holds the block shape or the
single-launch row shape to an earlier build).  The library is the one PLSVO_HIP_LIB names (default: pl-svo_amd/libplsvo_hip.so):

    PLSVO_HIP_LIB=$PWD/pl-svo_amd/libplsvo_hip_parent.so python tools/poseopt_ab_dump.py parent.npz
    python tools/poseopt_ab_dump.py tree.npz && cmp parent.npz tree.npz

Shapes: poseopt_threads 16 with the row refill off, 16 with it on, 64, 256.  Passes per shape, each run twice (the second run takes the
launch order refreshed from the first): poseopt_refill_cases.mixed_batch(P, 41); the same with one frame of the 10-argument overload
(n_iter_ref = 5); the first again with the iteration trace on.  Every shape runs in a child process of its own under a time limit."""
import hashlib, importlib, io, os, subprocess, sys, zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("rows", 16, False), ("rows_refill", 16, True), ("block64", 64, True), ("block256", 256, True))
STEP_SECONDS = 180
TRACE_CAP = 12


def run_shape(name, threads, refill, out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    P = importlib.import_module("pl-svo_amd")
    import poseopt_refill_cases as C
    jobs = C.mixed_batch(P, 41)
    ref = list(jobs)
    ref[17] = P.poseopt_job_from_frame(P.synth.make_poseopt_frame(79, 120, 40), n_iter_ref=5)
    ctx = C.make_ctx(P, PLSVO_POSEOPT_REFILL_MIN=4, PLSVO_POSEOPT_REORDER_MIN=4)
    arrays = {}
    try:
        ctx.set_launch_shapes(poseopt_threads=threads)
        ctx.set_poseopt_refill(refill)
        for tag, batch, trace in (("plain", jobs, 0), ("ref", ref, 0), ("trace", jobs, TRACE_CAP)):
            ctx.poseopt_set_trace(trace)
            ctx.poseopt_stage(batch)
            for run in range(2):
                s = C.snapshot(ctx, len(batch))
                key = f"{name}/{tag}/{run}/"
                for f in C.RESULT_FIELDS:
                    arrays[key + f] = np.frombuffer(b"".join(np.asarray(getattr(r, f)).tobytes() for r in s["res"]), np.uint8)
                arrays[key + "pose_records"] = np.frombuffer(s["recs"].tobytes(), np.uint8)
                arrays[key + "work"] = np.array(s["work"], np.uint64)
                arrays[key + "refill_frames"] = np.array([s["refill"]], np.int64)
                if trace:
                    logs, counts = [], []
                    for j in range(len(batch)):
                        log = (P.abi.PoseOptIterLog * trace)()
                        n = P.capi.C.c_int(0)
                        ctx._chk(ctx.L.plsvo_poseopt_fetch_trace(ctx.h, j, log, trace, P.capi.C.byref(n)))
                        counts.append(n.value)
                        logs.append(bytes(log)[:n.value * P.capi.C.sizeof(P.abi.PoseOptIterLog)])
                    arrays[key + "trace"] = np.frombuffer(b"".join(logs), np.uint8)
                    arrays[key + "trace_records"] = np.array(counts, np.int64)
        ctx.poseopt_set_trace(0)
    finally:
        ctx.close()
    np.savez(out, **arrays)
    print(f"{name}: {len(arrays)} arrays, refill took {int(arrays[name + '/plain/1/refill_frames'][0])} frames of the plain batch", flush=True)


def main(out):
    parts = {}
    for name, threads, refill in SHAPES:
        part = f"{out}.{name}.part.npz"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, part], timeout=STEP_SECONDS)
        if r.returncode != 0:
            raise SystemExit(f"poseopt_ab_dump: shape {name} ended with status {r.returncode}; nothing further is run")
        with np.load(part) as z:
            parts.update({k: z[k] for k in z.files})
        os.remove(part)
    # (np.savez stamps every member with the time of day: the members are written here with a fixed date, in sorted order, uncompressed)
    with zipfile.ZipFile(out, "w", zipfile.ZIP_STORED) as zf:
        for k in sorted(parts):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(parts[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
    print(f"{out}: {len(parts)} arrays, sha256 {hashlib.sha256(open(out, 'rb').read()).hexdigest()}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--shape":
        run_shape(*next(s for s in SHAPES if s[0] == sys.argv[2]), sys.argv[3])
    elif len(sys.argv) == 2:
        main(sys.argv[1])
    else:
        raise SystemExit(__doc__)
