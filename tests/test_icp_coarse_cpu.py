"""Rule C18 on the CPU (no GPU): the specification (perception_amd/icp_coarse.py), the host entries of the library that restate it
(cd_icp_coarse_subsample, the setter's argument checks, the struct size) and the stage planning of
perception_amd/csrc/icp_coarse_plan.hpp through its stand-alone program icp_coarse_plan_check, plain and built with
-fsanitize=address,undefined."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from perception_amd import capi, icp_coarse as IC

CSRC = os.path.join(ROOT, "perception_amd", "csrc")
OK, INVALID_ARG, CAPACITY, FEW = 0, -1, -2, -5      # cuboid_hip.h
ALIGN = 16                                           # COARSE_REGION_ALIGN
EYE = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]


# ---- the specification -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, s, want", [(5, 2, [0, 2, 4]), (6, 2, [0, 2, 4]), (7, 2, [0, 2, 4, 6]), (5, 3, [0, 3]), (6, 3, [0, 3]), (7, 3, [0, 3, 6]),
                                        (129, 64, [0, 64, 128]), (192, 64, [0, 64, 128]), (193, 64, [0, 64, 128, 192])])
def test_subsample(n, s, want):
    """p[j s], j = 0 .. ceil(n / s) - 1.  (min_points is its least legal value where that keeps the set eligible; the sets of five
    to seven points are below any legal min_points, so the index rule is read off with the gate open.)"""
    got = IC.indices(n, s)
    assert got.dtype == np.int32 and list(got) == want and len(got) == -(-n // s)
    m = 3 * s
    if n >= m:
        assert list(IC.subsample(n, s, m)) == want
        assert list(capi.icp_coarse_subsample(n, s, m)) == want
    else:
        assert len(IC.subsample(n, s, m)) == 0 and len(capi.icp_coarse_subsample(n, s, m)) == 0


@pytest.mark.parametrize("s, m", [(2, 6), (2, 40), (5, 15), (5, 61), (64, 192), (64, 2048)])
def test_eligibility_edge_and_the_library_equals_the_rule(s, m):
    assert not IC.eligible(m - 1, s, m) and IC.eligible(m, s, m)
    for n in (0, 1, m - 1, m, m + 1, m + s - 1, m + s, 7 * m + 3):
        want = IC.subsample(n, s, m)
        got = capi.icp_coarse_subsample(n, s, m)
        assert got.dtype == np.int32 and np.array_equal(got, want), (n, s, m)
        assert len(want) == (0 if n < m else -(-n // s))
        if len(want):
            assert want[-1] <= n - 1 < want[-1] + s     # the last point taken is the last one the stride reaches
    lib = capi.load_library()
    assert lib.cd_icp_coarse_subsample(m, s, m, None, 0) == -(-m // s)         # the count alone
    count, out = capi.icp_coarse_subsample(m + s, s, m, capacity=1)            # more than the buffer holds: nothing written
    assert count == -(-(m + s) // s) and out is None


def test_settings_the_setter_takes():
    ok = [(0, 0), (0, -5), (2, 6), (2, 7), (64, 192), (5, 1000)]
    bad = [(1, 100), (-2, 100), (65, 1000), (2, 5), (64, 191), (3, 0), (2, -6)]
    for s, m in ok:
        assert IC.setting_ok(s, m)
    for s, m in bad:
        assert not IC.setting_ok(s, m)
        assert len(IC.subsample(10000, s, m)) == 0 and len(capi.icp_coarse_subsample(10000, s, m)) == 0
    assert capi.load_library().cd_icp_coarse_struct_size() == C.sizeof(capi.CdIcpCoarseStats) == 32
    assert capi.CD_ICP_COARSE_STRIDE_MAX == IC.STRIDE_MAX and (capi.CD_COARSE_NOT_ELIGIBLE, capi.CD_COARSE_USED, capi.CD_COARSE_FELL_BACK) == \
        (IC.NOT_ELIGIBLE, IC.USED, IC.FELL_BACK)
    assert IC.CD_ERR_FEW_CORRESPONDENCES == capi.CD_ERR_FEW_CORRESPONDENCES
    # (without a context the setter and the getters refuse; with one: tests/test_gpu_icp_coarse.py)
    lib = capi.load_library()
    assert lib.cd_set_icp_coarse(None, 2, 6) == INVALID_ARG and lib.cd_get_icp_coarse(None, None, None) == INVALID_ARG
    assert lib.cd_get_cluster_coarse_stats(None, 0, 0, 0, None) == INVALID_ARG


def test_fall_back_predicate():
    T = np.eye(4, dtype=np.float32)
    assert not IC.fall_back(0, T)
    assert IC.fall_back(1, T)                       # a stopped state
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 7, 15):
            X = T.copy()
            X.ravel()[at] = bad
            assert IC.fall_back(0, X)


def test_two_levels_hand_over_and_fall_back():
    """two_level with a recording stand-in for the ICP: which sets are registered, from which guesses, and what the stats say."""
    pts = np.arange(30, dtype=np.float32).reshape(10, 3)
    G = np.full((4, 4), 7, np.float32)
    Tc = np.full((4, 4), 3, np.float32)

    def runner(stop_coarse, Tcoarse):
        calls = []

        def run(p, g):
            calls.append((p.copy(), g))
            coarse = len(p) < len(pts)
            return dict(T=Tcoarse if coarse else np.eye(4, dtype=np.float32), iterations=4 if coarse else 9, converged=0 if coarse and stop_coarse else 1,
                        fitness=0.25 if coarse else 0.5, stopped=int(coarse and stop_coarse))
        return run, calls

    run, calls = runner(False, Tc)
    fine, st = IC.two_level(pts, 3, 9, run, lambda p: G)
    assert [len(c[0]) for c in calls] == [4, 10] and np.array_equal(calls[0][0], pts[[0, 3, 6, 9]]) and calls[0][1] is G
    assert np.array_equal(calls[1][1], Tc) and fine["iterations"] == 9
    assert st == IC.CoarseStats(4, 4, 1, OK, 0.25, IC.USED)
    run, calls = runner(True, Tc)
    fine, st = IC.two_level(pts, 3, 9, run, lambda p: G)
    assert calls[1][1] is G and st == IC.CoarseStats(4, 4, 0, FEW, 0.25, IC.FELL_BACK)
    bad = Tc.copy()
    bad[1, 2] = np.nan
    run, calls = runner(False, bad)
    fine, st = IC.two_level(pts, 3, 9, run, lambda p: G)
    assert calls[1][1] is G and st == IC.CoarseStats(4, 4, 1, OK, 0.25, IC.FELL_BACK)
    run, calls = runner(False, Tc)
    fine, st = IC.two_level(pts, 3, 11, run, lambda p: G)       # not eligible
    assert len(calls) == 1 and len(calls[0][0]) == 10 and calls[0][1] is G and st == IC.NO_STATS
    # a guess per set (rule C13): each level asks for the guess of the set it registers
    run, calls = runner(True, Tc)
    IC.two_level(pts, 3, 9, run, lambda p: len(p))
    assert [c[1] for c in calls] == [4, 10]


# ---- icp_coarse_plan.hpp through its program ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["", "-fsanitize=address,undefined"], ids=["plain", "sanitized"])
def check_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("icp_coarse") / "icp_coarse_plan_check")
    cmd = ["g++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
           "-Wno-unknown-pragmas"] + ([request.param] if request.param else []) + [os.path.join(CSRC, "icp_coarse_plan_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def plan(exe, tmp_path, setting, capacity, clusters, extra=()):
    """clusters: (n, src_off, tpl_m, slot, frame) in order -> the program's JSON"""
    lines = ["setting %d %d" % setting, "capacity %d" % capacity] + ["cluster %d %d %d %d %d" % c for c in clusters] + list(extra)
    path = os.path.join(str(tmp_path), "case.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return json.loads(r.stdout)


def expected_plan(setting, clusters):
    """The plan by the rule: eligible problems in order, packed from the first aligned point behind the stage's clusters."""
    s, m = setting
    end = max([off + max(n, 0) for n, off, _, _, _ in clusters] or [0])
    begin = -(-end // ALIGN) * ALIGN
    at, coarse, gather, hand = begin, [], [], []
    for k, (n, off, tpl_m, slot, frame) in enumerate(clusters):
        idx = IC.subsample(n, s, m)
        if len(idx) == 0 or tpl_m <= 0:
            hand.append([-1, 0])
            continue
        hand.append([len(coarse), len(idx)])
        coarse.append([at, len(idx), frame, k, 1000 * slot, tpl_m, 0, slot])
        gather.append([off, at, len(idx), s])
        assert off + int(idx[-1]) < off + n          # the last read stays inside the cluster
        at += len(idx)
    return dict(begin=begin, end=end, needed=at if coarse else end, coarse=coarse, gather=gather, hand=hand)


MIXED = [(100, 0, 500, 0, 0), (39, 100, 500, 0, 0), (40, 139, 500, 0, 0), (41, 4096, 700, 1, 1), (2, 4137, 700, 1, 1), (90, 4139, 0, 2, 1), (77, 8192, 700, 1, 2)]


@pytest.mark.parametrize("name, setting, clusters", [
    ("empty", (2, 40), []),
    ("none", (2, 101), MIXED),
    ("off", (0, 0), MIXED),
    ("all", (3, 40), [c for c in MIXED if c[0] >= 40 and c[2] > 0]),
    ("mixed", (2, 40), MIXED),
    ("stride64", (64, 192), [(191, 0, 9, 0, 0), (192, 191, 9, 0, 0), (193, 383, 9, 0, 0), (1000, 576, 9, 0, 0)]),
])
def test_plan(check_exe, tmp_path, name, setting, clusters):
    w = expected_plan(setting, clusters)
    out = plan(check_exe, tmp_path, setting, 1 << 20, clusters)
    assert out["status"] == OK
    assert (out["region_begin"], out["capacity_needed"], out["n_eligible"]) == (w["begin"], w["needed"], len(w["coarse"]))
    assert out["coarse"] == w["coarse"] and out["gather"] == w["gather"] and out["hand"] == w["hand"]
    assert out["max_n_coarse"] == max([c[1] for c in w["coarse"]] or [0])
    if name in ("empty", "none", "off"):
        assert out["n_eligible"] == 0 and out["coarse"] == []
    if name == "all":
        assert out["n_eligible"] == len(clusters) > 0
    if name == "mixed":        # the template-less problem and the small ones stay out; the eligible ones keep their order
        assert [h[0] for h in out["hand"]] == [0, -1, 1, 2, -1, -1, 3]
    # the coarse region lies behind every cluster, and its sets do not overlap
    for (a, n, *_), (b, *_rest) in zip(out["coarse"], out["coarse"][1:] + [[out["capacity_needed"]]]):
        assert a >= w["end"] and a + n == b


def test_plan_capacity_edge(check_exe, tmp_path):
    w = expected_plan((2, 40), MIXED)
    assert plan(check_exe, tmp_path, (2, 40), w["needed"], MIXED)["status"] == OK
    out = plan(check_exe, tmp_path, (2, 40), w["needed"] - 1, MIXED)
    assert out["status"] == CAPACITY and out["capacity_needed"] == w["needed"]
    # no eligible problem: no capacity is asked for, however small the buffers
    assert plan(check_exe, tmp_path, (2, 101), 0, MIXED)["status"] == OK
    # a region that an IcpCluster's 32-bit offset cannot address
    big = [(1 << 30, 0, 9, 0, 0), (1 << 30, 1 << 30, 9, 0, 0)]
    out = plan(check_exe, tmp_path, (2, 6), 1 << 40, big)
    assert out["status"] == CAPACITY and out["capacity_needed"] == (1 << 31) + (1 << 30)


def test_plan_program_agrees_with_the_rule_on_hand_over_subsample_and_settings(check_exe, tmp_path):
    def state(status, converged, T):
        return "state %d %d %s" % (status, converged, " ".join(repr(float(v)) for v in T))
    nan7, inf0, ninf15 = list(EYE), list(EYE), list(EYE)
    nan7[7], inf0[0], ninf15[15] = float("nan"), float("inf"), float("-inf")
    extra = [state(OK, 1, EYE), state(OK, 0, EYE), state(-7, 1, EYE), state(OK, 1, nan7), state(OK, 1, inf0), state(OK, 1, ninf15),
             "subsample 193 64 192 4", "subsample 193 64 192 3", "subsample 191 64 192 8", "subsample 7 2 6 4", "subsample 100 1 3 100",
             "subsample 100 2 5 100", "subsample 12 5 15 0", "ok 0 0", "ok 2 6", "ok 2 5", "ok 64 192", "ok 65 500", "ok 1 100"]
    out = plan(check_exe, tmp_path, (2, 40), 0, [], extra)
    assert out["handover"] == [[OK, 0], [FEW, 1], [-7, 1], [OK, 1], [OK, 1], [OK, 1]]
    assert [bool(fb) for _, fb in out["handover"]] == [IC.fall_back(0, EYE), IC.fall_back(1, EYE), True, IC.fall_back(0, nan7), IC.fall_back(0, inf0),
                                                        IC.fall_back(0, ninf15)]
    assert out["subsample"] == [[4, 0, 64, 128, 192], [4], [0], [4, 0, 2, 4, 6], [0], [0], [0]]
    assert out["ok"] == [1, 1, 0, 1, 0, 0] == [int(IC.setting_ok(s, m)) for s, m in ((0, 0), (2, 6), (2, 5), (64, 192), (65, 500), (1, 100))]


# ---- icp_plan.hpp's defaulted input: per-problem guesses already on the device ----------------------------------------------------
@pytest.fixture(scope="module")
def stage_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("icp_plan_c18") / "icp_plan_check")
    subprocess.run(["g++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                    "-Wno-unknown-pragmas", "-fsanitize=address,undefined", os.path.join(CSRC, "icp_plan_check.cpp"), "-o", exe], check=True)
    return exe


def stage_plan(exe, tmp_path, lines):
    path = os.path.join(str(tmp_path), "stage.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return json.loads(r.stdout)


def test_fine_stage_plans_per_problem_guesses(stage_plan_exe, tmp_path):
    """The fine stage of rule C18: whatever the guess mode, the sources are moved per problem (guess_indexing 2) by a table of
    16 floats per problem, the states start from the call's own guess, and k_icp_lat's direct mode - which reads the host
    states - is off.  Without the input, and with it 0, the plan is today's."""
    lattice = ["slot 0 3 1 0"] + ["cluster %d %d 0 5000 0" % (n, f) for f, n in enumerate((900, 40, 2, 700))]
    base = stage_plan(stage_plan_exe, tmp_path, lattice)
    assert base["plan"]["lat_direct"] == 1 and base["plan"]["guess_need"] == 0 and "moved_by" not in base["plan"]
    off = stage_plan(stage_plan_exe, tmp_path, lattice + ["device_guesses 0"])
    assert off["plan"].pop("moved_by") == -1 and off["plan"].pop("device_guesses") == 0 and off == base
    on = stage_plan(stage_plan_exe, tmp_path, lattice + ["device_guesses 1"])
    p = on["plan"]
    assert (p["device_guesses"], p["moved_by"], p["lat_direct"], p["guess_need"], p["max_n"]) == (1, 2, 0, 16 * 4, 900)
    assert p["n_lat"] == base["plan"]["n_lat"] == 3 and on["states"] == base["states"] and on["work"] == base["work"]      # the drivers are who they were
    # a guess mode of the call: its guess stays in the states (what a problem that falls back starts from), the table is per problem
    frames = stage_plan(stage_plan_exe, tmp_path, lattice + ["use_guess 2", "guess_frames 4"])
    fine = stage_plan(stage_plan_exe, tmp_path, lattice + ["use_guess 2", "guess_frames 4", "device_guesses 1"])
    assert frames["plan"]["guess_need"] == 16 * 4 and fine["plan"]["guess_need"] == 16 * 4 and fine["plan"]["moved_by"] == 2
    assert fine["states"] == frames["states"] and fine["states"][1][6] != 0
    short = stage_plan(stage_plan_exe, tmp_path, lattice + ["use_guess 2", "guess_frames 3", "device_guesses 1"])
    assert short["status"] == INVALID_ARG                       # the call's own check stays
    single = stage_plan(stage_plan_exe, tmp_path, lattice + ["use_guess 1", "device_guesses 1"])
    assert single["plan"]["guess_need"] == 16 * 4 and single["plan"]["moved_by"] == 2 and single["states"][0][6][0] == -1.0
    cluster = stage_plan(stage_plan_exe, tmp_path, lattice + ["use_guess 4", "device_guesses 1"])
    assert cluster["plan"]["guess_need"] == 16 * 4 and cluster["plan"]["moved_by"] == 2 and cluster["plan"]["guess_mode"] == 4
