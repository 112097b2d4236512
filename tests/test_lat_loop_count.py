"""tools/lat_loop_count.py on this tree (compiles k_icp_lat.hip to assembly, no GPU): the resource budget of every k_icp_lat
instantiation and the vector instructions of one LAT_ITER pass on the path a three-face template takes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lat_loop_count.py"), "--json"], check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def test_every_instantiation_fits_four_waves_per_simd(report):
    """128 VGPRs is what __launch_bounds__(..., 4 waves per SIMD) allows; a spill or scratch costs far more than any instruction
    saved in the pass (profiles/r05_ab_vgpr.txt)."""
    assert len(report["resources"]) == 26          # 13 launch shapes, bounded and unbounded
    for name, r in report["resources"].items():
        assert r["vgpr_count"] <= 128 and r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)


def test_the_pass_of_a_three_face_template(report):
    """The face loop's pass had 217 vector instructions (counted by this tool on the commit before lat_nearest_axes); the
    one-face-per-axis form has to stay at least 30 below that, without a mask select."""
    for name, r in report["loop"].items():
        assert r["v_bfi_b32"] == 0 and r["v_f64"] == 32, (name, r)
        assert r["valu"] <= 217 - 30, (name, r)
