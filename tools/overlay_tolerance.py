"""Where the pixel tolerance of the overlay's behaviour test (tests/test_gpu_overlay.py) comes from: the CPU oracle alone, no GPU.

For every single-box synth frame (synth.frame(i, k_obj=1)) of the range, the oracle's chain (oracle.oracle_py.process_frame,
default parameters and template) gives a pose; rule C11's restatement (perception_amd/overlay.py) projects its box with the
camera synth renders with, and overlay.corner_error_px measures how far the drawn corners lie from the projection of
synth.truth_poses - the largest per-axis distance over the eight corners, minimised over the box's 180-degree symmetries.
Prints one line per frame and the largest value over the accepted frames; the test's tolerance is that value plus one pixel
(truncation), DESIGN.md rule C11.

  python tools/overlay_tolerance.py --frames 16
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def synth_P():
    """CameraInfo.P of synth's pinhole (the depth and colour images of synth.depth_frame are registered: E = identity)."""
    from perception_amd import synth
    fx, fy, cx, cy = synth.depth_camera_params()
    return (fx, 0.0, cx, 0.0, 0.0, fy, cy, 0.0, 0.0, 0.0, 1.0, 0.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=16, help="synth frames 0 .. frames - 1, one box each")
    args = ap.parse_args()
    from oracle import oracle_py as O
    from perception_amd import capi, overlay, synth, templates
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    prm = capi.default_params()
    P = synth_P()
    worst = 0.0
    for i in range(args.frames):
        res = O.process_frame(synth.frame(i, k_obj=1), prm, tpl)["result"]
        truth = synth.truth_poses(synth.scene_for(i, k_obj=1))[0]
        if res.n_clusters != 1 or not res.clusters[0].accepted:
            print("frame %2d: clusters %d, not accepted - left out" % (i, res.n_clusters))
            continue
        c, drawn = overlay.project(np.array(res.clusters[0].pose), P=P, dims=synth.CUBOID_DIMS)
        err = overlay.corner_error_px(c, truth, P=P, dims=synth.CUBOID_DIMS) if drawn else float("inf")
        worst = max(worst, err)
        print("frame %2d: accepted, fitness %.3e, corner error %.3f px" % (i, res.clusters[0].fitness, err))
    print("largest corner error over the accepted frames: %.3f px" % worst)


if __name__ == "__main__":
    main()
