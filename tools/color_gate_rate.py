"""Cost of the colour gate (rule C10, k_color_bbox) on config-3 batches (256 synth frames of 640 x 480, images resident in HBM,
one context, one batch at a time):

  * ms per batch of cd_color_bbox_batch_device alone (host clock around the synchronous call, and the spread);
  * frames/s of cd_process_depth_batch_device with the gate off, with CD_BBOX_PARAMS (one rectangle) and with CD_BBOX_COLOR,
    interleaved round by round in one process, and cd_timing's stage [0] (crop + voxel + deprojection + colour stage) of each;
  * beside them: the stage's compulsory read (3 bytes per pixel) against the copy ceiling profiles/ records (6.29 TB/s), and the
    CPU restatement's frames/s on one core (perception_amd/color_gate.py).

Prints one JSON line (and writes it with --out).  No pass / fail threshold.

  timeout -k 10 600 python tools/color_gate_rate.py --out profiles/color_gate_rate.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COPY_CEILING_TBPS = 6.29


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=256, help="frames per batch")
    ap.add_argument("--rounds", type=int, default=20, help="timed rounds (each runs every variant once)")
    ap.add_argument("--cpu-frames", type=int, default=8, help="frames of the CPU restatement's timing")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()

    from tools.depth_fed_rate import make_images
    F = args.frames
    depth, rgb = make_images(F)

    import torch
    from perception_amd import capi, color_gate, synth, templates
    if not torch.cuda.is_available():
        raise SystemExit("color_gate_rate.py needs an MI355X: the HIP path has no CPU fallback")
    W, H = synth.WIDTH, synth.HEIGHT
    P = W * H
    cam = capi.default_depth_camera()
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params()
    cam.depth_scale = synth.DEPTH_SCALE
    cam.color = capi.CD_COLOR_RGB8
    ctx = capi.Context(max_points=P, max_frames=F)
    ctx.set_template(0, templates.template_xyz32(**templates.DEFAULT_TEMPLATE))
    td = torch.from_numpy(depth.view(np.int16)).cuda().view(torch.uint16)
    tc = torch.from_numpy(rgb).cuda()
    torch.cuda.synchronize()

    off = capi.default_params()
    gated = capi.default_params()
    gated.bbox_enable = 1
    for i, v in enumerate([cam.fx, 0, cam.cx, 0, 0, cam.fy, cam.cy, 0, 0, 0, 1, 0]):
        gated.bbox_P[i] = v
    for i, v in enumerate((180, 180, 480, 460)):
        gated.bbox_rect[i] = v
    res = (capi.CdFrameResult * F)()

    def stage():
        ctx.color_bbox_batch_device(tc)

    def chain(prm, source):
        def run():
            ctx.set_bbox_source(source)
            ctx.process_depth_batch_device(td, tc, cam, prm, results=res)
            return ctx.timing().stage_ms[0], ctx.timing().stage_ms[4]
        return run

    variants = {"stage_alone": stage, "gate_off": chain(off, capi.CD_BBOX_PARAMS), "bbox_params": chain(gated, capi.CD_BBOX_PARAMS),
                "bbox_color": chain(gated, capi.CD_BBOX_COLOR)}
    for fn in variants.values():   # warm up every shape
        for _ in range(3):
            fn()
    wall = {k: [] for k in variants}
    stage0 = {k: [] for k in variants}
    total = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            a = time.perf_counter()
            r = fn()
            wall[name].append((time.perf_counter() - a) * 1e3)
            if r is not None:
                stage0[name].append(r[0])
                total[name].append(r[1])
    found = sum(b.found for b in ctx.frame_bboxes())
    ctx.set_bbox_source(capi.CD_BBOX_PARAMS)

    a = time.perf_counter()
    for f in range(args.cpu_frames):
        color_gate.color_bbox(rgb[f % F])
    cpu_fps = args.cpu_frames / (time.perf_counter() - a)

    def summary(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}

    read_mb = F * P * 3 / 1e6
    out = {"tool": "color_gate_rate", "frames_per_batch": F, "pixels_per_frame": P, "rounds": args.rounds,
           "stage_alone_ms_per_batch": summary(wall["stage_alone"]),
           "compulsory_read_MB_per_batch": read_mb, "copy_ceiling_TBps": COPY_CEILING_TBPS,
           "ms_at_copy_ceiling": read_mb / 1e6 / COPY_CEILING_TBPS * 1e3,
           "frames_found_last_color_batch": int(found),
           "cpu_restatement_frames_per_s_one_core": cpu_fps,
           "chain": {k: {"frames_per_s": F / (statistics.median(wall[k]) / 1e3), "wall_ms_per_batch": summary(wall[k]),
                         "stage0_ms": summary(stage0[k]), "device_total_ms": summary(total[k])}
                     for k in ("gate_off", "bbox_params", "bbox_color")},
           "note": "one context, one batch at a time (not bench.py's pipeline of batches in flight); wall = host clock around the "
                   "synchronous call; stage0 / device_total = cd_timing's HIP events"}
    ctx.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
