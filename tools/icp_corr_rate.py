"""What the ICP maximum correspondence distance (cd_set_icp_max_correspondence_distance, rule C8) costs: frames/s of one
context, unbounded against bounded, both tracking with a per-frame guess (CD_GUESS_PER_FRAME) as tests/test_gpu_icp_corr.py
does - single-object frames, each frame's guess its best pose of an unbounded pass moved by a seeded motion of <= 1 cm and
<= 2 degrees.  Two workloads: config 3 (default template, lattice search) and the object launch (leaf 0.001, threshold 0.01,
a scanned template, generic search).  The cost is reported, not gated.  Prints one JSON line (and writes it with --out).

  timeout -k 10 600 python tools/icp_corr_rate.py --out profiles/icp_corr_rate.json
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


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


def workload(name, tpl, prm, frames, dist, reps):
    from perception_amd import capi, synth
    F = len(frames)
    batch = np.stack(frames, 0)
    c = capi.Context(max_points=synth.WIDTH * synth.HEIGHT, max_frames=F)
    try:
        c.set_template(0, tpl)
        r0, _, _ = c.process_batch(batch, prm)
        rng = np.random.default_rng(21)
        guesses = np.empty((F, 4, 4), np.float32)
        for f in range(F):
            k = min(r0[f].n_clusters, capi.CD_MAX_CLUSTERS_PER_FRAME)
            T = np.array(min((r0[f].clusters[i] for i in range(k)), key=lambda r: r.fitness).T if k else np.eye(4).ravel(), np.float64).reshape(4, 4)
            P = np.eye(4)
            P[:3, :3] = rot(*np.deg2rad(rng.uniform(-2, 2, 3)))
            P[:3, 3] = rng.uniform(-0.01, 0.01, 3) / np.sqrt(3)
            guesses[f] = P @ T
        c.set_frame_guesses(guesses)
        prm.icp_use_guess = capi.CD_GUESS_PER_FRAME
        out = {"frames": F, "reps": reps, "max_correspondence_distance": dist}
        for tag, d in (("unbounded", None), ("bounded", dist)):
            c.set_icp_max_correspondence_distance(d)
            res, _, _ = c.process_batch(batch, prm)   # (warm-up)
            t0 = time.perf_counter()
            for _ in range(reps):
                res, _, _ = c.process_batch(batch, prm)
            dt = time.perf_counter() - t0
            pairs = [res[f].clusters[k] for f in range(F) for k in range(min(res[f].n_clusters, capi.CD_MAX_CLUSTERS_PER_FRAME))]
            out[tag] = {"frames_per_s": F * reps / dt, "icp_iterations_mean": float(np.mean([p.iterations for p in pairs])),
                        "pairs": len(pairs), "pairs_stopped_few_correspondences": int(sum(p.iterations == 0 and not p.converged for p in pairs)),
                        "icp_kernel_ms_last_batch": float(c.timing().icp_kernel_ms)}
        out["bounded_over_unbounded"] = out["bounded"]["frames_per_s"] / out["unbounded"]["frames_per_s"]
        return name, out
    finally:
        c.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dist", type=float, default=0.01, help="maximum correspondence distance of the bounded runs (m)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from perception_amd import capi, pcd, synth, templates
    frames = [synth.frame(i, k_obj=1) for i in range(args.frames)]
    res = {"workload": "one context, per-frame guess, single-object synth frames, %d frames per batch" % args.frames}
    prm = capi.default_params()
    k, v = workload("config3", templates.template_xyz32(**templates.DEFAULT_TEMPLATE), prm, frames, args.dist, args.reps)
    res[k] = v
    prm = capi.default_params()
    prm.leaf_size, prm.plane_distance_threshold = 0.001, 0.01
    tpl = pcd.read_xyz(os.path.join(ROOT, "tests", "golden", "eraser_ascii_tf.pcd"))
    k, v = workload("object_launch", tpl, prm, frames, args.dist, args.reps)
    res[k] = v
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
