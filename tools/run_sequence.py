"""Run the frame-to-frame harness (pl-svo_amd/sequence.py) on the GPU and write the trajectory in the reference
harness's format (app/run_pipeline.cpp:433-451: `timestamp tx ty tz qx qy qz qw` of T_f_w^-1).
With mapping (default on) 40 % of the point landmarks start as depth-filter seeds and structure optimisation runs at every
fifth frame, so all of align / reproject / match / pose-opt / structure-opt / seed update are exercised.
With --distortion k1,k2,p1,p2[,k3] every frame is first turned into the raw frame of a radial-tangential camera with those
coefficients (synth.distort_image) and rectified on the device into its pyramid slot (plsvo_hip_rectify_build_pyramid), the way
run_pipeline.cpp undistorts each raw frame before addImage.
With --detect (off by default; needs mapping) every keyframe also runs the corner detector on its pyramid slot (plsvo_hip_detect_fast)
and the corners become depth-filter seeds (sequence.seeds_from_corners) that the following frames update: seeds that come from the image.
With --kf-select (off by default; needs mapping) the keyframe stage runs on the device (plsvo_close_keyframes, plsvo_keyframe_decide): a
frame plays the keyframe when FrameHandlerMono::needNewKf says so instead of every fifth, and the JSON line lists the keyframe frames.
With --map-candidates (off by default) reprojection and matching take their candidates from the map-candidate stage (plsvo_candidates_*):
the overlap keyframes' features, one visit per landmark, the closest-view observation as the reference patch.
With --bootstrap-klt nothing of the above runs: the sequence's first frames play KltHomographyInit up to the homography on the device
(sequence.klt_bootstrap: corners of frame 0, a KLT second frame per image until the disparity gate passes) and the reports are printed.
usage: python tools/run_sequence.py [--bootstrap-klt] [--distortion k1,k2,p1,p2[,k3]] [--detect] [--kf-select] [--map-candidates] [--cell-select] [--kf-insert] [--seed-candidates] [--seeds-resident] [--image-seeds host|device] [--structopt-resident] [--compact room|always] [--keystage host|device] [--align host|device] [--relocalize host|device] [--lm-room N] [out.txt] [n_frames] [seed] [mapping 0|1]"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = importlib.import_module("pl-svo_amd")
seqm = importlib.import_module("pl-svo_amd.sequence")

argv = sys.argv[1:]
distortion = None
if "--distortion" in argv:
    k = argv.index("--distortion")
    distortion = [float(v) for v in argv[k + 1].split(",")]
    if len(distortion) not in (4, 5):
        raise SystemExit("--distortion takes k1,k2,p1,p2[,k3]")
    del argv[k:k + 2]
detect = "--detect" in argv
if detect:
    argv.remove("--detect")
kf_select = "--kf-select" in argv
if kf_select:
    argv.remove("--kf-select")
map_candidates = "--map-candidates" in argv
if map_candidates:
    argv.remove("--map-candidates")
cell_select = "--cell-select" in argv              # with --map-candidates: one candidate per cell and the resident pose optimiser
if cell_select:
    argv.remove("--cell-select")
    map_candidates = True
kf_insert = "--kf-insert" in argv                  # with --cell-select and mapping: keyframes are inserted into the resident tables, not staged anew
if kf_insert:
    argv.remove("--kf-insert")
seed_candidates = "--seed-candidates" in argv      # with --kf-insert: a converged seed is appended to the resident tables (plsvo_candidates_add), not staged
if seed_candidates:
    argv.remove("--seed-candidates")
seeds_resident = "--seeds-resident" in argv        # with --seed-candidates: the seed lists are staged once and updated, erased and handed over on the device (plsvo_seeds_*)
if seeds_resident:
    argv.remove("--seeds-resident")
image_seeds = None                                 # with --seeds-resident: a keyframe's corners become point seeds of the resident lists, on the device or through the host
if "--image-seeds" in argv:
    i = argv.index("--image-seeds")
    image_seeds = argv[i + 1]
    del argv[i:i + 2]
structopt_resident = "--structopt-resident" in argv   # with --cell-select and mapping: the structure optimisation runs on the resident tables every tracked frame
if structopt_resident:
    argv.remove("--structopt-resident")
compact, lm_room = None, None                      # with --seed-candidates: the resident tables close up over their deleted point rows behind every keyframe
if "--compact" in argv:
    i = argv.index("--compact")
    compact = argv[i + 1]
    del argv[i:i + 2]
align = None
if "--align" in argv:                              # host | device: the alignment job from the previous frame's selection (needs --map-candidates --cell-select)
    i = argv.index("--align")
    align = argv[i + 1]
    del argv[i:i + 2]
keystage = None
if "--keystage" in argv:                           # host | device: the keyframe stage with live key points (needs --kf-select --cell-select --kf-insert)
    i = argv.index("--keystage")
    keystage = argv[i + 1]
    del argv[i:i + 2]
relocalize = None
if "--relocalize" in argv:                         # host | device: the tracking gates and relocalizeFrame (needs --align and --keystage of the same transport)
    i = argv.index("--relocalize")
    relocalize = argv[i + 1]
    del argv[i:i + 2]
if "--lm-room" in argv:                            # landmark rows reserved per kind instead of one per seed of the sequence
    i = argv.index("--lm-room")
    lm_room = int(argv[i + 1])
    del argv[i:i + 2]
bootstrap_klt = "--bootstrap-klt" in argv
if bootstrap_klt:
    argv.remove("--bootstrap-klt")
sys.argv = sys.argv[:1] + argv

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "gpurun_out", "trajectory.txt")
n_frames = int(sys.argv[2]) if len(sys.argv) > 2 else 30
seed = int(sys.argv[3]) if len(sys.argv) > 3 else 7
mapping = bool(int(sys.argv[4])) if len(sys.argv) > 4 else True
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
seq = seqm.make_sequence(seed, n_frames, 640, 480, 200, 80, total=0.35)      # 35 % of the scene depth + 0.09 rad over the whole run
ctx = P.capi.Context(0)
if bootstrap_klt:
    # the synthetic plane is smooth between its landmarks: a FAST threshold of 7 finds the corners the default of 20 does not (as --image-seeds)
    reports, tracks = seqm.klt_bootstrap(seqm.HipBackend(ctx), seq["images"], seq["cam"], detect=dict(fast_threshold=7, detection_threshold=2.0))
    print(json.dumps({"bootstrap_klt": reports, "frames_played": len(reports), "tracks": len(tracks["px_ref"]),
                      "disparity_min_max": [float(tracks["disparity"].min()), float(tracks["disparity"].max())] if len(tracks["disparity"]) else None}))
    ctx.close()
    sys.exit(0)
rectify = None
if distortion is not None:
    fx, fy, cx, cy, w, h = seq["cam"]
    seq = dict(seq, images=[P.synth.distort_image(img, dict(fx=fx, fy=fy, cx=cx, cy=cy, d=distortion)) for img in seq["images"]])
    rectify = P.abi.pinhole_radtan(w, h, fx, fy, cx, cy, distortion)
res = seqm.run_sequence(seqm.HipBackend(ctx, rectify=rectify), seq, mapping=mapping, detect=detect, kf_select=kf_select, map_candidates=map_candidates, cell_select=cell_select, kf_insert=kf_insert,
                        seed_candidates=seed_candidates, seeds_resident=seeds_resident, image_seeds=image_seeds, structopt_resident=structopt_resident, compact=compact, lm_room=lm_room, keystage=keystage, align=align, relocalize=relocalize,
                        image_seed_params=dict(fast_threshold=7, detection_threshold=2.0) if image_seeds else None)
n = P.trajectory.write_trajectory(out, ["%.6f" % (0.05 * k) for k in range(n_frames)], [r["T"] for r in res], [r["cov"] for r in res])
err = seqm.pose_errors(res, seq)
print(json.dumps({"frames": n_frames, "lines_written": n, "trajectory": out, "max_rot_err_rad": max(e[0] for e in err),
                  "max_trans_err_m": max(e[1] for e in err), "matched_points_last": res[-1]["n_matched_pt"], "matched_segments_last": res[-1]["n_matched_seg"],
                  "mapping": mapping, "distortion": distortion, "landmarks_first_last": [res[1].get("n_known"), res[-1].get("n_known")],
                  "seeds_first_last": [res[1].get("n_seeds"), res[-1].get("n_seeds")],
                  **({"image_seeds_last": res[-1].get("n_image_seeds"), "image_seeds_converged": res[-1].get("n_image_seeds_converged")} if detect else {}),
                  **({"keyframes": [k for k, r in enumerate(res) if r.get("is_kf")], "overlap_last": res[-1].get("n_overlap"),
                      "depth_mean_last": res[-1].get("depth_mean")} if kf_select else {}),
                  **({"seed_candidates_per_frame": [r.get("n_seed_candidates", 0) for r in res[1:]],
                      "seed_candidates_mean": sum(r.get("n_seed_candidates", 0) for r in res[1:]) / max(len(res) - 1, 1)} if seed_candidates else {}),
                  **({"relocalize": relocalize, "stages": [r["stage"] for r in res[1:]], "gates": [r["gate"] for r in res[1:]]} if relocalize else {}),
                  **({"keystage": keystage, "key_pts_last": res[-1]["key_pts"].tolist()} if keystage else {}),
                  **({"compacted_rows_per_keyframe": [r["n_compacted_pt"] for r in res if "n_compacted_pt" in r]} if compact else {})}))
ctx.close()
