"""icp_step_row == icp_step on the host, before anything runs on a GPU: perception_amd/csrc/icp_solve_row_check.cpp emulates the
row of 16 lanes with arrays and compares every byte of the outgoing state and the return value on 1e7 random moment sets (each
unbounded and bounded), the structured ones its header lists, and sets built to take each convergence branch."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "perception_amd", "csrc")


def test_row_step_equals_single_lane_step_on_the_host():
    subprocess.run(["make", "-C", CSRC, "icp_solve_row_check"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(CSRC, "icp_solve_row_check"), "10000000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    ok, sets, stop, limit, eps, abs_, rel, open_, rank2 = r.stdout.split()
    assert ok == "ok" and int(sets) >= 2 * 10000000 - 600000      # (a few random sets are skipped: see kind 7 of random_sets)
    # every exit of the step was taken, often
    assert min(int(v) for v in (stop, limit, eps, abs_, rel, open_, rank2)) >= 100000, r.stdout
