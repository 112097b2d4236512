"""The small clustering tier (CL_TIER_CAP / CL_TIER_SLOTS, kernels.hpp) is sized from the bench frames: their object clouds, as
the oracle extracts them, must fit its point capacity and occupy well under the 3/4 of its cell table that may fill - otherwise
every bench batch would pay the redo with the next tier.  Eight of the 256 bench scenes are counted here (all 256: at most 4306
points in at most 800 cells)."""
import os
import re

import numpy as np

from perception_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tier_constants():
    src = open(os.path.join(ROOT, "perception_amd", "csrc", "kernels.hpp")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (CL_TIER_CAP|CL_TIER_SLOTS|CL_TIER_THREADS) = (\d+);", src)}


def test_bench_frames_fit_the_small_tier(O, template):
    c = tier_constants()
    assert set(c) == {"CL_TIER_CAP", "CL_TIER_SLOTS", "CL_TIER_THREADS"}
    prm = capi.default_params()
    prm.rgb_offset = 12
    edge = np.float32(prm.cluster_tolerance / np.sqrt(3.0) * (1.0 - 1.0 / 1024.0))
    inv = np.float32(1.0) / edge
    worst_points = worst_cells = worst_coord = 0
    for i in range(0, 256, 32):
        fr = synth.frame(i)
        obj = O.process_frame(fr, prm, template, want_clouds=True)["objects"]
        x, z = fr[:, 0], fr[:, 2]
        with np.errstate(invalid="ignore"):
            kept = (z >= prm.crop_z_min) & (z <= prm.crop_z_max) & (x >= prm.crop_x_min) & (x <= prm.crop_x_max)
        origin = fr[kept, :3].min(0)                      # the cell origin of the kernels: the cropped cloud's minimum
        cell = np.floor((obj - origin) * inv).astype(np.int64)
        worst_points = max(worst_points, len(obj))
        worst_cells = max(worst_cells, len(np.unique(cell[:, 0] + (cell[:, 1] << 10) + (cell[:, 2] << 20))))
        worst_coord = max(worst_coord, int(cell.max()))
    print("8 bench frames: at most %d object points, %d occupied cells, cell coordinate %d" % (worst_points, worst_cells, worst_coord))
    assert 0 < worst_points <= c["CL_TIER_CAP"]
    assert 0 < worst_cells <= c["CL_TIER_SLOTS"] // 4 * 3 // 3 * 2      # two thirds of what the table may hold: room for other scenes
    assert worst_coord <= 1018
