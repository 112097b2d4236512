"""What rule C14 (perception_amd/verify.py) says about the poses of the CPU oracle, and - with --gpu - what the check
costs on the device.

CPU (default, no GPU): every synth.depth_frame(i) of the range is deprojected by rule C7 and run through the oracle's chain
(oracle.oracle_py.process_frame, default parameters and template).  For every cluster the report holds `accepted`, the fitness,
the rule's record against the frame's depth image (tolerance 0.01 m, dims synth.CUBOID_DIMS, the defaults of
cd_default_verify_params) and the pose error against the nearest of synth.truth_poses, minimised over the box's 180-degree
flips; also the records of the truth poses themselves and of the first box's truth pose perturbed (yawed by 90 degrees, turned 90
degrees about the box x axis, shifted 1 cm along the box z axis, flipped by 180 degrees).  Prints the table and writes
profiles/verify_report.json.  tests/test_verify_cpu.py asserts what is printed here.

  python tools/verify_report.py --frames 0 16

GPU (--gpu, needs an MI355X): a 256-frame cd_process_depth_batch_device on depth images resident in HBM, then
cd_verify_last_results_device on its poses: host wall time of each call around a device synchronisation, warm-up calls first,
median / min / max over --reps calls, added to the JSON under "gpu".

  timeout -k 10 600 python tools/verify_report.py --gpu --reps 20
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "verify_report.json")


def synth_camera():
    from perception_amd import capi, synth
    cam = capi.default_depth_camera()
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params()
    cam.depth_scale = synth.DEPTH_SCALE
    return cam


def pose_error(pose, truths):
    """(translation error in mm, rotation error in degrees, index) against the nearest truth pose, the rotation minimised over the
    identity and the three 180-degree turns that map a cuboid onto itself."""
    from perception_amd.overlay import SYMMETRIES
    T = np.asarray(pose, np.float64).reshape(4, 4)
    k = int(np.argmin([np.linalg.norm(T[:3, 3] - G[:3, 3]) for G in truths]))
    G = truths[k]
    best = 180.0
    for sgn in SYMMETRIES:
        c = (np.trace((G[:3, :3] * np.asarray(sgn)[None, :]).T @ T[:3, :3]) - 1.0) / 2.0
        best = min(best, float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))))
    return float(np.linalg.norm(T[:3, 3] - G[:3, 3]) * 1e3), best, k


def _plain(rec):
    from perception_amd import verify
    out = {k: int(rec[k]) for k in ("verified", "passed") + verify.COUNTS}
    out["score"] = float(rec["score"])
    return out


def perturbed(T):
    """The perturbations of a truth pose the table lists, by name."""
    def mul(R=np.eye(3), t=(0.0, 0.0, 0.0)):
        D = np.eye(4)
        D[:3, :3], D[:3, 3] = R, t
        return T @ D
    return {"yawed by 90 degrees": mul(R=np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])),
            "turned 90 degrees about the box x axis": mul(R=np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])),
            "shifted 1 cm along the box z axis": mul(t=(0.0, 0.0, 0.01)),
            "flipped by 180 degrees": mul(R=np.diag([-1.0, -1.0, 1.0]))}


def cpu_report(first, last):
    from oracle import oracle_py as O
    from perception_amd import capi, synth, templates, verify
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    prm = capi.default_params()
    cam = synth_camera()
    dims = synth.CUBOID_DIMS
    clusters, truths, variants = [], [], []
    for i in range(first, last):
        depth = synth.depth_frame(i)[0]
        res = O.process_frame(verify.depth_cloud(depth, cam), prm, tpl)["result"]
        gt = synth.truth_poses(synth.scene_for(i))
        for k in range(min(res.n_clusters, capi.CD_MAX_CLUSTERS_PER_FRAME)):
            cr = res.clusters[k]
            rec = verify.record(verify.verify_box(depth, cam, np.array(cr.pose), dims))
            mm, deg, box = pose_error(np.array(cr.pose), gt)
            clusters.append(dict(frame=i, cluster=k, accepted=int(cr.accepted), fitness=float(cr.fitness), nearest_box=box,
                                 translation_error_mm=mm, rotation_error_deg=deg, **_plain(rec)))
        for b, T in enumerate(gt):
            truths.append(dict(frame=i, box=b, **_plain(verify.record(verify.verify_box(depth, cam, T, dims)))))
        for name, P in perturbed(gt[0]).items():
            variants.append(dict(frame=i, what=name, **_plain(verify.record(verify.verify_box(depth, cam, P, dims)))))
    return dict(tool="verify_report", frames=[first, last], tolerance=verify.DEFAULT_TOLERANCE, dims=list(dims),
                min_score=verify.DEFAULT_MIN_SCORE, min_agree=verify.DEFAULT_MIN_AGREE, clusters=clusters, truth=truths,
                perturbed_truth=variants)


def print_table(rep):
    def span(rows, key="score"):
        v = [r[key] for r in rows]
        return "%.3f .. %.3f" % (min(v), max(v)) if v else "-"
    cl = rep["clusters"]
    for r in cl:
        print("frame %2d cluster %d: accepted %d fitness %.3e  passed %d score %.3f  hit %6d agree %6d through %6d occluded %5d "
              "invalid %4d  error %.1f mm %.1f deg" % (r["frame"], r["cluster"], r["accepted"], r["fitness"], r["passed"], r["score"],
                                                       r["n_hit"], r["n_agree"], r["n_through"], r["n_occluded"], r["n_invalid"],
                                                       r["translation_error_mm"], r["rotation_error_deg"]))
    good = [r for r in cl if r["accepted"] and r["passed"]]
    bad = [r for r in cl if r["accepted"] and not r["passed"]]
    rej = [r for r in cl if not r["accepted"]]
    print("accepted by the fitness test, passed:      %3d  score %s" % (len(good), span(good)))
    print("accepted by the fitness test, NOT passed:  %3d  score %s  %s" % (len(bad), span(bad), [(r["frame"], r["cluster"]) for r in bad]))
    print("rejected by the fitness test:              %3d  score %s  passed %d  %s" % (len(rej), span(rej), sum(r["passed"] for r in rej), [(r["frame"], r["cluster"]) for r in rej]))
    tr = rep["truth"]
    print("truth poses:                               %3d  score %s  through %d .. %d  passed %d" % (
        len(tr), span(tr), min(r["n_through"] for r in tr), max(r["n_through"] for r in tr), sum(r["passed"] for r in tr)))
    for name in dict.fromkeys(r["what"] for r in rep["perturbed_truth"]):
        rows = [r for r in rep["perturbed_truth"] if r["what"] == name]
        print("first truth pose %-40s score %s  passed %d of %d" % (name + ":", span(rows), sum(r["passed"] for r in rows), len(rows)))


def gpu_report(reps, warmup, n_frames):
    import torch
    from perception_amd import capi, synth, templates
    if not torch.cuda.is_available():
        raise SystemExit("verify_report.py --gpu needs an MI355X: the HIP path has no CPU fallback")
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    cam = synth_camera()
    prm = capi.default_params()
    depth = np.stack([synth.depth_frame(i % 16)[0] for i in range(16)])
    depth = np.ascontiguousarray(depth[np.arange(n_frames) % 16])
    ctx = capi.Context(max_points=synth.WIDTH * synth.HEIGHT, max_frames=n_frames)
    ctx.set_template(0, tpl)
    td = torch.from_numpy(depth.view(np.int16)).cuda().view(torch.uint16)
    torch.cuda.synchronize()
    vprm = capi.verify_params(dims=synth.CUBOID_DIMS)

    def timed(fn, n):
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            a = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - a) * 1e3)
        return out, r

    fused = lambda: ctx.process_depth_batch_device(td, None, cam, prm)
    check = lambda: ctx.verify_last_results(td, cam, capi.CD_VERIFY_ALL, vprm)
    timed(fused, warmup)
    t_fused, res = timed(fused, reps)
    timed(check, warmup)
    t_check, boxes = timed(check, reps)
    rec = capi.verify_records(boxes)
    stat = lambda t: dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)), reps=len(t))
    out = dict(frames=n_frames, boxes=int(sum(min(res[f].n_clusters, capi.CD_MAX_CLUSTERS_PER_FRAME) for f in range(n_frames))),
               verified=int(rec["verified"].sum()), passed=int(rec["passed"].sum()), pixels_hit=int(rec["n_hit"].sum()),
               cd_process_depth_batch_device=stat(t_fused), cd_verify_last_results_device=stat(t_check), warmup=warmup,
               note="host wall time per call around a device synchronisation; depth images resident in HBM; CD_VERIFY_ALL")
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, nargs=2, default=(0, 16), metavar=("FIRST", "END"), help="synth depth frames FIRST .. END - 1")
    ap.add_argument("--gpu", action="store_true", help="only the device timing (added to the JSON written before)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="frames of the timed batch")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    rep = json.load(open(args.out)) if args.gpu and os.path.exists(args.out) else {}
    if args.gpu:
        rep["gpu"] = gpu_report(args.reps, args.warmup, args.batch)
        print(json.dumps(rep["gpu"]))
    else:
        rep = cpu_report(*args.frames)
        print_table(rep)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rep) + "\n")


if __name__ == "__main__":
    main()
