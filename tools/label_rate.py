"""What the point labels of rule C15 cost after a fused call (one MI355X, one context, bench.py's 256 synth frames of 640 x 480 as
a depth batch, everything resident in HBM):

  (a) cd_label_depth_last_device alone
  (b) cd_label_depth_last_device followed by cd_tint_labels_batch_device on the frames' rgb8 images

Host clock around each call (both end with a synchronisation of the context's stream), medians of --reps after a warm-up.  The
labels of the first run are checked against the numpy restatement on --check frames.  Prints one JSON line (and writes it with
--out).

  timeout -k 10 600 python tools/label_rate.py --out profiles/label_rate.json
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/label_rate.py --reps 5
  python tools/label_rate.py --kernel-stats DIR/run_kernel_stats.csv --out profiles/label_rate.json
      (no GPU: adds the k_label_* / k_tint_labels rows of the trace to the JSON written before)
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def add_kernel_stats(path, out):
    res = json.load(open(out)) if os.path.exists(out) else {}
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if any(k in r.get("Name", "") for k in ("k_label_voxel_keys", "k_label_voxel_classes", "k_label_points", "k_tint_labels"))]
    if not rows:
        raise SystemExit("no k_label_* row in %s" % path)
    res["kernel_trace"] = {r["Name"].split("(")[0].split("::")[-1].split("<")[0] + ("<depth>" if "<true>" in r["Name"] else ""):
                           {"calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) / 1e6, "min_ms": float(r["MinNs"]) / 1e6,
                            "max_ms": float(r["MaxNs"]) / 1e6} for r in rows}
    line = json.dumps(res)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--check", type=int, default=2, help="frames whose labels are compared with perception_amd/point_labels.py")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, help="no run: add the label kernels' rows of this rocprofv3 stats CSV to --out")
    args = ap.parse_args()
    if args.kernel_stats:
        return add_kernel_stats(args.kernel_stats, args.out)

    from tools.depth_fed_rate import make_images
    import torch
    from perception_amd import capi, point_labels, synth, templates
    if not torch.cuda.is_available():
        raise SystemExit("label_rate.py needs an MI355X: the HIP path has no CPU fallback")
    F, W, H = args.frames, synth.WIDTH, synth.HEIGHT
    depth, rgb = make_images(F)
    cam = capi.default_depth_camera()
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params()
    cam.depth_scale = synth.DEPTH_SCALE
    cam.color = capi.CD_COLOR_NONE
    prm = capi.default_params()
    ctx = capi.Context(max_points=W * H, max_frames=F)
    ctx.set_template(0, templates.template_xyz32(**templates.DEFAULT_TEMPLATE))
    d_depth = torch.from_numpy(depth.view(np.int16)).cuda().view(torch.uint16)
    d_rgb0 = torch.from_numpy(rgb).cuda()
    d_rgb = d_rgb0.clone()
    d_lab = torch.zeros((F, H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def fused():
        t = time.perf_counter()
        pi = np.empty((F, W * H), np.int32)
        lb = np.empty((F, W * H), np.int32)
        res = ctx.process_depth_batch_device(d_depth, None, cam, prm, plane_inliers=pi, labels=lb)
        return res, pi, lb, (time.perf_counter() - t) * 1e3

    res, pi, lb, _ = fused()
    ctx.label_depth_last(d_depth, cam, out=d_lab)          # warm-up: buffers, first touch
    ctx.tint_labels(d_rgb, d_lab)
    got = d_lab[:args.check].cpu().numpy()
    for f in range(min(args.check, F)):
        r = res[f]
        vox = ctx.frame_cloud(f, capi.CD_CLOUD_VOXELS, 16, -1)[:, :3].copy().view(np.float32)
        obj = ctx.frame_cloud(f, capi.CD_CLOUD_OBJECTS, 16, -1)[:, :3].copy().view(np.float32)
        want = point_labels.labels_of_frame(point_labels.deproject(depth[f], cam), prm, r.n_voxels, pi[f][:r.n_plane], vox, obj, lb[f][:r.n_objects])
        if not np.array_equal(got[f].reshape(-1), want):
            raise SystemExit("label_rate: frame %d differs from the numpy restatement" % f)
    fused_ms = [fused()[3] for _ in range(3)]

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    label_ms = [timed(lambda: ctx.label_depth_last(d_depth, cam, out=d_lab)) for _ in range(args.reps)]

    def both():
        ctx.label_depth_last(d_depth, cam, out=d_lab)
        ctx.tint_labels(d_rgb, d_lab)
    both_ms = [timed(both) for _ in range(args.reps)]
    px = F * W * H
    hist = torch.bincount(d_lab.reshape(-1).to(torch.int64), minlength=16)[:16].cpu().tolist()
    out = {"tool": "label_rate", "frames_per_batch": F, "pixels_per_frame": W * H, "reps": args.reps,
           "label_ms_median": statistics.median(label_ms), "label_ms_min": min(label_ms), "label_ms_max": max(label_ms),
           "label_tint_ms_median": statistics.median(both_ms), "label_tint_ms_min": min(both_ms), "label_tint_ms_max": max(both_ms),
           "fused_call_with_index_readback_ms": fused_ms,
           "label_bytes": px * 3, "label_bytes_note": "2 B read + 1 B written per pixel", "tint_bytes": px * 7,
           "label_GBps_at_median": px * 3 / statistics.median(label_ms) / 1e6,
           "voxels_per_frame_mean": float(np.mean([res[f].n_voxels for f in range(F)])),
           "labels_0_to_15": hist, "checked_frames": min(args.check, F)}
    ctx.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
