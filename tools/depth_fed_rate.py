"""Host-fed rate of the three forms a D435 frame can cross PCIe in (config-3 batches: 256 frames of 640 x 480, the synth
scene, BatchPipeline from PINNED host memory, the same number of batches in flight for each):

  (a) cloud       16-byte x y z rgb records through cd_process_batch (bench.py's host-fed leg)     4.92 MB / frame
  (b) depth+rgb8  16UC1 + registered rgb8 through cd_process_depth_batch                           1.54 MB / frame
  (c) depth       16UC1 alone through cd_process_depth_batch                                       0.61 MB / frame

(a) runs on the organized cloud that (b)'s images deproject to (cd_depth_to_cloud), so the records of (a) and (b) must be
identical: checked in the run.  Prints one JSON line (and writes it with --out).

  timeout -k 10 600 python tools/depth_fed_rate.py --batches 60 --out profiles/depth_fed_rate.json
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
      python tools/depth_fed_rate.py --legs b --batches 8 --inflight 1
  python tools/depth_fed_rate.py --kernel-stats DIR/run_kernel_stats.csv --out profiles/depth_fed_rate.json
      (no GPU: adds the k_deproject line of the trace to the JSON written before)
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_images(count):
    """depth (F, H, W) uint16 and rgb8 (F, H, W, 3) of synth frames 0 .. count-1, rendered on host threads."""
    from concurrent.futures import ThreadPoolExecutor
    from perception_amd import synth
    depth = np.empty((count, synth.HEIGHT, synth.WIDTH), np.uint16)
    rgb = np.empty((count, synth.HEIGHT, synth.WIDTH, 3), np.uint8)

    def work(i):
        depth[i], rgb[i] = synth.depth_frame(i)

    with ThreadPoolExecutor(max(1, min(16, count))) as ex:
        list(ex.map(work, range(count)))
    return depth, rgb


def add_kernel_stats(path, out):
    """The k_deproject row of a rocprofv3 --stats kernel table, added to the JSON at `out`."""
    res = json.load(open(out)) if os.path.exists(out) else {}
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "k_deproject" in r.get("Name", "")]
    if not rows:
        raise SystemExit("no k_deproject row in %s" % path)
    r = rows[0]
    avg_ns = float(r["AverageNs"])
    px = res.get("frames_per_batch", 256) * res.get("pixels_per_frame", 640 * 480)
    res["k_deproject_trace"] = {
        "calls": int(r["Calls"]), "avg_ms": avg_ns / 1e6, "min_ms": float(r["MinNs"]) / 1e6, "max_ms": float(r["MaxNs"]) / 1e6,
        "bytes_per_batch": px * (2 + 3 + 16), "TBps": px * (2 + 3 + 16) / avg_ns / 1e3,
        "note": "rocprofv3 --kernel-trace --stats of a run of leg (b) alone, one batch in flight: depth + rgb8 in, 16-byte records "
                "out, %d-frame batches; TBps = those bytes over the average duration" % res.get("frames_per_batch", 256)}
    line = json.dumps(res)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=256, help="frames per batch")
    ap.add_argument("--inflight", type=int, default=5, help="batches in flight (one context and host thread each)")
    ap.add_argument("--batches", type=int, default=None, help="timed batches per leg (default 4 x inflight)")
    ap.add_argument("--legs", default="abc", help="which of the legs a, b, c to run")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    ap.add_argument("--kernel-stats", default=None, help="no run: add the k_deproject row of this rocprofv3 stats CSV to --out")
    args = ap.parse_args()
    if args.kernel_stats:
        return add_kernel_stats(args.kernel_stats, args.out)

    os.environ.setdefault("GPU_MAX_HW_QUEUES", "10")   # as bench.py's config 3: a queue per batch in flight
    F, M = args.frames, max(1, args.inflight)
    K = args.batches or 4 * M
    depth, rgb = make_images(F)

    import torch
    from perception_amd import batch, capi, synth, templates
    if not torch.cuda.is_available():
        raise SystemExit("depth_fed_rate.py needs an MI355X: the HIP path has no CPU fallback")
    P = synth.WIDTH * synth.HEIGHT
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    cam = capi.default_depth_camera()
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params()
    cam.depth_scale = synth.DEPTH_SCALE
    cam_rgb, cam_d = capi.CdDepthCamera.from_buffer_copy(cam), capi.CdDepthCamera.from_buffer_copy(cam)
    cam_rgb.color, cam_d.color = capi.CD_COLOR_RGB8, capi.CD_COLOR_NONE
    prm = capi.default_params()
    prm.rgb_offset = 12
    pipe = batch.BatchPipeline(P, F, {0: tpl}, inflight=M)

    def pump(submit, k):
        """k batches, all waited for: (records of the last one, seconds)"""
        a = time.perf_counter()
        futs = [submit() for _ in range(k)]
        last = [f.result()[0] for f in futs][-1]
        torch.cuda.synchronize()
        return last, time.perf_counter() - a

    legs = {}
    records = {}
    bytes_per_frame = {"a": P * 16, "b": P * (2 + 3), "c": P * 2}
    if "a" in args.legs:
        cloud = np.stack([pipe.contexts[0].depth_to_cloud(cam_rgb, depth[f], rgb[f]) for f in range(F)]).view(np.float32)
        pin_cloud = torch.from_numpy(cloud).pin_memory()
    pin_depth = torch.from_numpy(depth.view(np.int16)).pin_memory()
    pin_rgb = torch.from_numpy(rgb).pin_memory()
    submit = {
        "a": lambda: pipe.submit(pin_cloud.data_ptr(), 16, P, F, prm, host=True),
        "b": lambda: pipe.submit_depth(pin_depth.data_ptr(), pin_rgb.data_ptr(), F, cam_rgb, prm),
        "c": lambda: pipe.submit_depth(pin_depth.data_ptr(), None, F, cam_d, prm),
    }
    names = {"a": "cloud_16B", "b": "depth_rgb8", "c": "depth_only"}
    for leg in "abc":
        if leg not in args.legs:
            continue
        pump(submit[leg], M)                                  # buffers, first touch
        rec, s = pump(submit[leg], K)
        records[leg] = rec
        mb = F * bytes_per_frame[leg] / 1e6
        legs[names[leg]] = {"frames_per_s": F * K / s, "MB_per_batch": mb, "GBps_uploaded": mb * K / s / 1e3, "batches": K, "seconds": s}
    out = {"tool": "depth_fed_rate", "frames_per_batch": F, "pixels_per_frame": P, "batches_in_flight": M,
           "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "legs": legs}
    if "a" in records and "b" in records:
        out["records_b_equal_a"] = bool(np.array_equal(records["a"], records["b"]))
    if "a" in legs:
        for leg in ("depth_rgb8", "depth_only"):
            if leg in legs:
                out["speedup_%s_over_cloud" % leg] = legs[leg]["frames_per_s"] / legs["cloud_16B"]["frames_per_s"]
    pipe.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    if out.get("records_b_equal_a") is False:
        raise SystemExit("depth_fed_rate: the records of (b) differ from those of (a)")


if __name__ == "__main__":
    main()
