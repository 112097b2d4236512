"""What the pose information (cd_set_pose_info, rule C23) says about accepted results, and what it costs.  GPU.

Three legs, each a child process of its own under its own time limit, the next only when the one before ended well:
  synth    synth.frame(0 .. --synth-frames - 1), the launch template, default parameters with icp_use_guess = CD_GUESS_CLUSTER, the
           mode on at the default range and a support of 1: for every accepted result the least eigenvalue lambda_0 and, for the
           candidate supports 2 .. 64, n_constrained - against the number of faces the cluster actually shows.  A cluster shows a
           face of its box (the nearest of synth.truth_poses by centroid) when at least --face-min of its points as extracted lie
           nearer to that face than to any other and within 4 mm of it.  Then, per candidate support, how many results with fewer
           than three faces it calls fully constrained and how many three-face results it does not.
  config3  --config3-frames bench frames, the launch template, default parameters
  object   --object-frames bench frames at the object launch's resolution (leaf 1 mm, plane threshold 10 mm), the launch template
In the last two one context runs the fused call (host-fed cd_process_batch) with the mode off and on ALTERNATELY, --reps times each
after a warm-up of each, and prints the medians, minima and maxima of cd_timing.stage_ms[3] (the ICP stage, which the step's launch
is part of: on minus off is what the step costs), of the device total and of the wall time.

  python tools/pose_info_report.py
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SUPPORTS = (2.0, 4.0, 8.0, 16.0, 32.0, 64.0)


def frames_of(n):
    from concurrent.futures import ThreadPoolExecutor
    from perception_amd import synth
    with ThreadPoolExecutor(16) as ex:       # (numpy releases the GIL in its array loops)
        return np.ascontiguousarray(np.stack(list(ex.map(synth.frame, range(n)))))


def faces_shown(points, box, face_min):
    """How many faces of `box` (R, c, half: box -> camera) hold at least face_min of the points."""
    p = (points.astype(np.float64) - box["c"]) @ box["R"]                  # camera -> box
    gap = np.abs(np.abs(p) - box["half"][None, :])                         # distance to the nearer face of each axis
    a = np.argmin(gap, axis=1)
    near = gap[np.arange(len(p)), a] <= 0.004
    side = (p[np.arange(len(p)), a] > 0).astype(int)
    counts = np.bincount((2 * a + side)[near], minlength=6)
    return int((counts >= face_min).sum())


def synth_leg(n_frames, face_min):
    from perception_amd import capi, synth, templates
    frames = frames_of(n_frames)
    prm = capi.default_params()
    prm.rgb_offset = 12
    prm.icp_use_guess = capi.CD_GUESS_CLUSTER
    ctx = capi.Context(max_points=frames.shape[1], max_frames=n_frames)
    ctx.set_template(0, templates.template_xyz32(**templates.DEFAULT_TEMPLATE))
    ctx.set_pose_info(True, capi.CD_POSE_INFO_RANGE_DEFAULT, 1.0)
    ctx.process_batch(frames, prm)
    rows = []                                                              # (faces shown, lambda_0, eigenvalues, n_in)
    for f in range(n_frames):
        boxes = synth.scene_for(f)["boxes"]
        res, info = ctx.cluster_results(f), ctx.cluster_pose_info(f)
        for k, (r, i) in enumerate(zip(res, info)):
            if not r.accepted or i.status != 0:
                continue
            pts = ctx.cluster_points(f, k, aligned=False)[:, :3]
            box = min(boxes, key=lambda b: np.linalg.norm(pts.mean(axis=0) - b["c"]))
            rows.append((faces_shown(pts, box, face_min), list(i.eigenvalues), i.n_in))
    ctx.close()
    print("GPU, synth.frame(0..%d), the launch template, CD_GUESS_CLUSTER: %d accepted results; a face counts from %d points" % (n_frames - 1, len(rows), face_min))
    print("| faces shown | results | lambda_0 min / median / max | lambda_1 median | kept points median |")
    print("|---|---|---|---|---|")
    for nf in sorted({r[0] for r in rows}):
        sel = [r for r in rows if r[0] == nf]
        l0 = [r[1][0] for r in sel]
        print("| %d | %d | %.3g / %.3g / %.3g | %.3g | %d |" % (nf, len(sel), min(l0), float(np.median(l0)), max(l0), float(np.median([r[1][1] for r in sel])),
                                                           int(np.median([r[2] for r in sel]))))
    print("\n| min_support | n_constrained = 6 among results of fewer than three faces | n_constrained < 6 among three-face results | n_constrained histogram (0 .. 6) |")
    print("|---|---|---|---|")
    for s in SUPPORTS:
        ncon = [sum(1 for v in r[1] if v >= s) for r in rows]
        few = [c for r, c in zip(rows, ncon) if r[0] < 3]
        full = [c for r, c in zip(rows, ncon) if r[0] >= 3]
        print("| %g | %d of %d | %d of %d | %s |" % (s, sum(1 for c in few if c == 6), len(few), sum(1 for c in full if c < 6), len(full),
                                                  " ".join(str(ncon.count(v)) for v in range(7))))


def cost_leg(leg, n_frames, reps):
    from perception_amd import capi, templates
    frames = frames_of(n_frames)
    prm = capi.default_params()
    prm.rgb_offset = 12
    if leg == "object":
        prm.leaf_size = 0.001
        prm.plane_distance_threshold = 0.01
    ctx = capi.Context(max_points=frames.shape[1], max_frames=n_frames)
    ctx.set_template(0, templates.template_xyz32(**templates.DEFAULT_TEMPLATE))

    def call(on):
        ctx.set_pose_info(on, capi.CD_POSE_INFO_RANGE_DEFAULT, capi.CD_POSE_INFO_MIN_SUPPORT_DEFAULT)
        t0 = time.perf_counter()
        ctx.process_batch(frames, prm)
        wall = (time.perf_counter() - t0) * 1e3
        tm = ctx.timing()
        out = dict(wall=wall, icp=float(tm.stage_ms[3]), total=float(tm.stage_ms[4]), iters=0, clusters=0, points=0)
        if on:
            res = [c for f in range(n_frames) for c in ctx.cluster_results(f)]
            out.update(clusters=len(res), points=sum(c.size for c in res), iters=sum(c.iterations for c in res))
        return out
    for on in (False, True):
        call(on)                                 # warm-up of each
    runs = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):                 # alternately: the settings share whatever else the machine is doing
            runs[on].append(call(on))
    last = runs[True][-1]
    print("GPU, %s leg: %d bench frames, leaf %g, %d interleaved calls each (host-fed cd_process_batch): %d clusters, %d points, %d ICP iterations in all"
          % (leg, n_frames, prm.leaf_size, reps, last["clusters"], last["points"], last["iters"]))
    print("| mode | ICP stage ms (stage_ms[3]) median / min / max | device ms (stage_ms[4]) median / min / max | wall ms median / min / max |")
    print("|---|---|---|---|")
    fmt = lambda v: "%.3f / %.3f / %.3f" % (float(np.median(v)), min(v), max(v))
    for on in (False, True):
        print("| %s | %s | %s | %s |" % ("on" if on else "off", fmt([r["icp"] for r in runs[on]]), fmt([r["total"] for r in runs[on]]), fmt([r["wall"] for r in runs[on]])))
    med = lambda on, key: float(np.median([r[key] for r in runs[on]]))
    cost, icp = med(True, "icp") - med(False, "icp"), med(False, "icp")
    per_iter = icp * last["clusters"] / max(last["iters"], 1)
    print("the step costs %.3f ms of stage [3] (on minus off, medians), %.3f ms of the device total; the stage's ICP runs %.1f iterations per cluster, so one "
          "iteration of every cluster is about %.3f ms of it\n" % (cost, med(True, "total") - med(False, "total"), last["iters"] / max(last["clusters"], 1), per_iter))
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--synth-frames", type=int, default=48)
    ap.add_argument("--face-min", type=int, default=10)
    ap.add_argument("--config3-frames", type=int, default=256)
    ap.add_argument("--object-frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--leg", choices=("synth", "config3", "object"), default=None, help="run one leg in this process")
    args = ap.parse_args()
    if args.leg == "synth":
        synth_leg(args.synth_frames, args.face_min)
        return 0
    if args.leg:
        cost_leg(args.leg, args.object_frames if args.leg == "object" else args.config3_frames, args.reps)
        return 0
    # each leg in a fresh child process under its own time limit; a leg that fails, faults or runs out of time ends the report
    for leg in ("synth", "config3", "object"):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--synth-frames", str(args.synth_frames), "--face-min", str(args.face_min),
               "--config3-frames", str(args.config3_frames), "--object-frames", str(args.object_frames), "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print("the %s leg ran out of its %d s: nothing further is started" % (leg, args.limit))
            return 124
        if r.returncode != 0:
            print("the %s leg ended with status %d: nothing further is started" % (leg, r.returncode))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
