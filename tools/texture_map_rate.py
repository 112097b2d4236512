"""The mapped depth call beside the registered one (config-3 batches: 256 frames of 640 x 480, the synth scene, device-resident
images, one context): stage [0] of cd_process_depth_batch_mapped_device (rule C12, k_texture_map) against stage [0] of
cd_process_depth_batch_device with colour (rule C7, k_deproject) on the SAME depth images.  The mapped leg uses the README's
colour camera 15 mm to the side and colour images rendered from it; the registered leg the images registered to the depth.
Prints one JSON line (and writes it with --out).

  timeout -k 10 600 python tools/texture_map_rate.py --out profiles/texture_map_rate.json
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/texture_map_rate.py --reps 6
  python tools/texture_map_rate.py --kernel-stats DIR/run_kernel_stats.csv --out profiles/texture_map_rate.json
      (no GPU: adds the k_texture_map and k_deproject lines of the trace to the JSON written before)

Algorithmic bytes per pixel: 2 in (depth) + 16 out (record) + 3 gathered per textured point for the mapping; 2 + 3 + 16 for the
registered deprojection.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DISTINCT = 16      # distinct synth frames, repeated to fill the batch (the kernels' time does not depend on the content)


def add_kernel_stats(path, out):
    res = json.load(open(out)) if os.path.exists(out) else {}
    px = res.get("frames_per_batch", 256) * res.get("pixels_per_frame", 640 * 480)
    share = res.get("textured_share", 0.0)
    per_px = {"k_texture_map": 2 + 16 + 3 * share, "k_deproject": 2 + 3 + 16}
    with open(path) as f:
        rows = list(csv.DictReader(f))
    for name, b in per_px.items():
        hit = [r for r in rows if name in r.get("Name", "")]
        if not hit:
            raise SystemExit("no %s row in %s" % (name, path))
        r = hit[0]
        avg_ns = float(r["AverageNs"])
        res[name + "_trace"] = {"calls": int(r["Calls"]), "avg_ms": avg_ns / 1e6, "min_ms": float(r["MinNs"]) / 1e6,
                                "max_ms": float(r["MaxNs"]) / 1e6, "bytes_per_pixel": b, "GBps": px * b / avg_ns}
    res["trace_note"] = ("rocprofv3 --kernel-trace --stats of a run of its own, both legs alternating on one context; GBps = the "
                         "algorithmic bytes of a batch over the average duration")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        return add_kernel_stats(a.kernel_stats, a.out)
    import torch
    from perception_amd import capi, synth, templates
    from perception_amd import texture_map as tm
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this is a measurement, there is nothing to fall back to")
    W, H, F = synth.WIDTH, synth.HEIGHT, a.frames
    cam = capi.default_depth_camera()
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params()
    cam.color = capi.CD_COLOR_RGB8
    cc = capi.color_camera(t=(0.015, 0.0, 0.0))
    depth = np.empty((DISTINCT, H, W), np.uint16)
    reg = np.empty((DISTINCT, H, W, 3), np.uint8)
    raw = np.empty((DISTINCT, cc.height, cc.width, 3), np.uint8)
    for i in range(DISTINCT):
        depth[i], reg[i] = synth.depth_frame(i)
        raw[i] = synth.render_color_camera(synth.scene_for(i), cc)[0]
    share = float(tm.project(depth, cam, cc)[3].mean())
    rep = (F + DISTINCT - 1) // DISTINCT
    td = torch.from_numpy(np.tile(depth.view(np.int16), (rep, 1, 1))[:F]).cuda()
    treg = torch.from_numpy(np.tile(reg, (rep, 1, 1, 1))[:F]).cuda()
    traw = torch.from_numpy(np.tile(raw, (rep, 1, 1, 1))[:F]).cuda()
    torch.cuda.synchronize()
    ctx = capi.Context(max_points=W * H, max_frames=F)
    ctx.set_template(0, templates.template_xyz32(**templates.DEFAULT_TEMPLATE))
    prm = capi.default_params()
    legs = {"registered": (treg, None), "mapped": (traw, cc)}
    stage0 = {k: [] for k in legs}
    total = {k: [] for k in legs}
    objects = {}
    for it in range(a.warmup + a.reps):
        for name, (col, ccam) in legs.items():          # alternating, so that both legs see the same machine
            res = ctx.process_depth_batch_device(td, col, cam, prm, color_camera=ccam)
            t = ctx.timing()
            if it >= a.warmup:
                stage0[name].append(float(t.stage_ms[0]))
                total[name].append(float(t.stage_ms[4]))
            objects[name] = int(sum(r.n_objects for r in res))
    out = {"frames_per_batch": F, "pixels_per_frame": W * H, "reps": a.reps, "textured_share": share,
           "stage0_ms": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in stage0.items()},
           "total_ms": {k: float(np.median(v)) for k, v in total.items()}, "n_objects": objects,
           "note": "stage [0] = deprojection / mapping + zero launch + crop + voxel grid; the mapped batch keeps only the textured "
                   "share of the pixels (CD_NOTEX_DROP), so its crop and voxel stages see fewer points"}
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
