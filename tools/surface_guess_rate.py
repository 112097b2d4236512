"""What the surface guess (icp_use_guess = CD_GUESS_SURFACE) does to the chain: frames/s, the ICP stage, iterations, acceptance
and pose error against synth.truth_poses, for the identity start (the default path) and the surface guess at sne thresholds
0.015 (surface_normal_estimation.launch) and 0.004.  Frames: one-box synth frames, synth.scene_for(i, k_obj=1) with the box's
yaw drawn uniformly over +-90 degrees instead of +-20 (R rebuilt as scene_for builds it), rendered by synth.render; the launch
template and leaf.  The rotation error is minimised over the box's four proper 180-degree symmetries.  Prints one JSON line
(and writes it with --out).

  timeout -k 10 900 python tools/surface_guess_rate.py --out profiles/surface_guess.json
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

SYMS = [np.diag(d) for d in ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))]


def scene(i, rng):
    from perception_amd import synth
    sc = synth.scene_for(i, k_obj=1)
    yaw = np.deg2rad(rng.uniform(-90.0, 90.0))
    ex = np.cos(yaw) * sc["e1"] + np.sin(yaw) * sc["e2"]
    ey = np.cross(sc["n"], ex)
    sc["boxes"][0]["R"] = np.stack([ex, ey, sc["n"]], axis=1)
    sc["boxes"][0]["yaw"] = yaw
    return sc


def rot_err_deg(Ra, Rb):
    best = 180.0
    for S in SYMS:
        c = (np.trace(Ra.T @ Rb @ S) - 1.0) / 2.0
        best = min(best, float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))))
    return best


def stats(v):
    v = np.asarray(v, np.float64)
    if v.size == 0:
        return None
    return {"mean": float(v.mean()), "median": float(np.median(v)), "p90": float(np.percentile(v, 90)), "max": float(v.max())}


def run(ctx, batches, truths, prm, reps):
    from perception_amd import capi
    for b in batches:   # (warm-up: every batch once)
        ctx.process_batch(b, prm)
    t0 = time.perf_counter()
    icp_ms = []
    for _ in range(reps):
        for b in batches:
            ctx.process_batch(b, prm)
            icp_ms.append(float(ctx.timing().stage_ms[3]))
    dt = time.perf_counter() - t0
    n_frames = sum(len(b) for b in batches)
    iters, accepted, n_cl, terr, rerr, sne_ok, guess_rerr = [], 0, 0, [], [], 0, []
    for bi, b in enumerate(batches):
        res, _, _ = ctx.process_batch(b, prm)
        sur = ctx.surface_results() if prm.icp_use_guess == capi.CD_GUESS_SURFACE else None
        for f in range(len(b)):
            r = res[f]
            T = truths[bi][f]
            k = min(r.n_clusters, capi.CD_MAX_CLUSTERS_PER_FRAME)
            cls = [r.clusters[j] for j in range(k)]
            n_cl += len(cls)
            accepted += sum(1 for c in cls if c.accepted)
            iters += [c.iterations for c in cls]
            if r.flags & capi.CD_FRAME_SURFACE_GUESS:
                sne_ok += 1
                G = capi.surface_guess(np.array(sur[1][f].Rt, np.float32)).astype(np.float64)
                guess_rerr.append(rot_err_deg(np.linalg.inv(G)[:3, :3], T[:3, :3]))
            if cls:
                best = min(cls, key=lambda c: c.fitness)
                P = np.array(best.pose).reshape(4, 4)
                terr.append(float(np.linalg.norm(P[:3, 3] - T[:3, 3])) * 1000.0)
                rerr.append(rot_err_deg(P[:3, :3], T[:3, :3]))
    terr = np.array(terr)
    return {
        "frames_per_s": n_frames * reps / dt,
        "icp_stage_ms_per_batch": float(np.mean(icp_ms)),
        "icp_iterations_mean": float(np.mean(iters)) if iters else None,
        "clusters": n_cl, "accepted_clusters": accepted,
        "sne_success_frames": sne_ok if prm.icp_use_guess == capi.CD_GUESS_SURFACE else None,
        "translation_error_mm": stats(terr), "rotation_error_deg": stats(rerr),
        "frames_over_10mm": int((terr > 10.0).sum()), "share_over_10mm": float((terr > 10.0).mean()) if terr.size else None,
        # sne's size-ordered axes against the truth before ICP: a guess more than 45 degrees off every symmetry of the box
        # has its axes swapped (out of scope here; recorded)
        "guess_rotation_error_deg": stats(guess_rerr),
        "guesses_axes_swapped": int(sum(e > 45.0 for e in guess_rerr)) if prm.icp_use_guess == capi.CD_GUESS_SURFACE else None,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256, help="frames per batch")
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from perception_amd import capi, synth, templates
    rng = np.random.default_rng(20190409)
    batches, truths = [], []
    for b in range(args.batches):
        scs = [scene(b * args.frames + i, rng) for i in range(args.frames)]
        batches.append(np.stack([synth.render(s) for s in scs], 0))
        truths.append([synth.truth_poses(s)[0] for s in scs])
        print("batch %d rendered" % b, file=sys.stderr, flush=True)
    ctx = capi.Context(max_points=synth.WIDTH * synth.HEIGHT, max_frames=args.frames)
    out = {"workload": "one context, %d batches of %d one-box synth frames, yaw uniform over +-90 deg, launch template and leaf"
                       % (args.batches, args.frames), "reps": args.reps}
    try:
        ctx.set_template(0, templates.template_xyz32(**templates.DEFAULT_TEMPLATE))
        prm = capi.default_params()
        out["identity"] = run(ctx, batches, truths, prm, args.reps)
        print("identity done", file=sys.stderr, flush=True)
        for thr in (0.015, 0.004):
            ctx.set_surface_distance_threshold(thr)
            prm = capi.default_params()
            prm.icp_use_guess = capi.CD_GUESS_SURFACE
            out["surface_%g" % thr] = run(ctx, batches, truths, prm, args.reps)
            print("surface %g done" % thr, file=sys.stderr, flush=True)
    finally:
        ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
