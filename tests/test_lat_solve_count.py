"""tools/lat_loop_count.py --solve on this tree (compiles a stand-alone probe of icp_step and icp_step_row to assembly, no GPU):
the row build's rotation body stays below the single-lane one by what the row solve achieved, and it is the SHORT form that is
counted - two IEEE divisions per rotation, the plain form behind its validity test."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured with this tool (`--solve --csrc <parent>/perception_amd/csrc`) on the parent commit: the sweep loop of the single-lane
# icp_step holds 743 vector instructions = 247.7 per rotation body (six IEEE float divisions and three IEEE square roots each);
# before the sweeps 411 (15 + 9 divisions), after them 488.
PARENT_ROTATION = 743 / 3.0
# The row build when it was written: 493 in the loop = 164.3 per rotation (before 99, after 243).
ACHIEVED = (743 - 493) / 3.0
SLACK = 5.0


@pytest.fixture(scope="module")
def report():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lat_loop_count.py"), "--solve", "--json"], check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])["solve"]


def test_rotation_body_of_the_row_build(report):
    lane, row = report["lane"], report["row"]
    print("rotation body: single lane %.1f, row %.1f vector instructions" % (lane["rotation"]["valu"], row["rotation"]["valu"]))
    assert row["rotation"]["valu"] <= PARENT_ROTATION - (ACHIEVED - SLACK), (row["rotation"], lane["rotation"])
    # the single-lane step is the parent's, untouched
    assert abs(lane["rotation"]["valu"] - PARENT_ROTATION) <= SLACK, lane["rotation"]


def test_the_short_forms_are_what_is_emitted(report):
    """Per rotation the short form keeps two IEEE divisions (d / t and the one of tau) and three hardware square roots; the
    other four divisions and the IEEE square roots only exist in the plain form, three copies of which sit behind the tests."""
    row = report["row"]
    assert row["loop"]["v_div_fixup_f32"] == 3 * 2 and row["loop"]["v_sqrt_f32"] == 3 * 3, row["loop"]
    assert row["plain_form_skipped"]["v_div_fixup_f32"] == 3 * 6 and row["plain_form_skipped"]["v_sqrt_f32"] == 3 * 3
    assert report["lane"]["loop"]["v_div_fixup_f32"] == 3 * 6


def test_straight_line_parts(report):
    """One double division for the 16 means and one float division for W before the sweeps, against 15 and 9."""
    lane, row = report["lane"], report["row"]
    assert (lane["before"]["v_div_fixup_f64"], lane["before"]["v_div_fixup_f32"]) == (15, 9)
    assert (row["before"]["v_div_fixup_f64"], row["before"]["v_div_fixup_f32"]) == (1, 1)
    assert row["before"]["valu"] < lane["before"]["valu"] and row["after"]["valu"] < lane["after"]["valu"]
