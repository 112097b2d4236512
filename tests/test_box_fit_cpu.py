"""The box fit (rule C24) on the CPU: the numpy specification (perception_amd/box_fit.py) on known answers and on every status, its
preconditions against the synthetic truth on the oracle's clusters, the host arithmetic of box_fit_math.hpp (box_fit_math_check,
plain and sanitized; the library's host calls) against the module bit for bit, and the names the header and capi.py export."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import box_fit_scenarios as S
from conftest import ROOT
from perception_amd import box_fit as BF, capi, synth

CSRC = os.path.join(ROOT, "perception_amd", "csrc")
NEW_SYMBOLS = ["cd_set_box_fit", "cd_get_box_fit", "cd_box_fit_struct_size", "cd_get_cluster_box_fits", "cd_box_fit_points", "cd_box_fit_host",
               "cd_box_fit_match"]
LEAF = 0.005
CONFIG5 = np.array([d[:3] for d in synth.CONFIG5_DIMS], np.float64)
CONFIG5_TOLERANCE = 0.0125     # half the smallest max-norm gap between two CONFIG5_DIMS rows


def fit(name):
    co, xyz, band = S.kernel_cases()[name]
    return BF.box_fit(co, xyz, band)


def test_header_and_capi_export_the_names():
    header = open(os.path.join(ROOT, "include", "cuboid_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS
    assert (capi.CD_BOX_FIT_BAND_DEFAULT, capi.CD_BOX_FIT_LDS_POINTS) == (BF.BAND_DEFAULT, BF.LDS_POINTS)
    assert re.search(r"#define\s+CD_BOX_FIT_BAND_DEFAULT\s+0\.006\b", header) and re.search(r"#define\s+CD_BOX_FIT_LDS_POINTS\s+%d\b" % BF.LDS_POINTS, header)
    assert C.sizeof(capi.CdBoxFit) == 216 and capi.load_library().cd_box_fit_struct_size() == 216
    assert (BF.CD_OK, BF.CD_ERR_INVALID_ARG, BF.CD_ERR_CAPACITY, BF.CD_ERR_NO_MODEL, BF.CD_ERR_FEW_CORRESPONDENCES) == \
        (capi.CD_OK, capi.CD_ERR_INVALID_ARG, capi.CD_ERR_CAPACITY, capi.CD_ERR_NO_MODEL, capi.CD_ERR_FEW_CORRESPONDENCES)
    for m in ("set_box_fit", "box_fit_setting", "cluster_box_fits", "box_fit_points"):
        assert callable(getattr(capi.Context, m))


def test_the_two_config5_rows_closest_to_each_other_are_twice_the_tolerance_apart():
    gaps = [np.abs(CONFIG5[i] - CONFIG5[j]).max() for i in range(5) for j in range(i)]
    assert abs(min(gaps) - 2 * CONFIG5_TOLERANCE) < 1e-15      # (the rows are decimal fractions: their differences round)


# ---- the specification on known answers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.KNOWN))
def test_lattice_rectangles_have_exact_answers(name):
    """Every coordinate is a multiple of 2^-10 and every floor exact: L, W, H, the hull, the rectangularity and the long axis follow
    from the lattice counts exactly; the centre within the few roundings of step 8 (1e-14 m)."""
    args = S.KNOWN[name]
    co, xyz, want = S.lattice_box(**args)
    r = BF.box_fit(co, xyz)
    assert (r["status"], r["n"], r["n_top"], r["hull_vertices"], r["overflow"], r["match_slot"]) == (BF.CD_OK, len(xyz), want["n_top"], 4, 0, -1)
    assert (r["dims"][0], r["dims"][1], r["dims"][2]) == (want["L"], want["W"], want["H"])
    assert r["height_ref"] == want["H"] and r["rectangularity"] == 1.0 and r["area"] == want["L"] * want["W"] and r["match_cost"] == 0.0
    P = r["pose"].reshape(4, 4)
    assert np.abs(P[:3, 3] - want["centre"]).max() <= 1e-14
    assert np.array_equal(P[:3, 2], want["nrm"]) and np.array_equal(P[3], [0, 0, 0, 1])
    # the long axis in (u, v): the side with more lattice steps, its u component positive
    la, lb = np.hypot(*args["step_a"]) * args["na"], np.hypot(*args["step_b"]) * args["nb"]
    ax = np.array(args["step_a"] if la >= lb else args["step_b"], np.float64)
    ax = ax if (ax[0] > 0 or (ax[0] == 0 and ax[1] > 0)) else -ax
    got_u, got_v = float(P[:3, 0] @ want["eu"]), float(P[:3, 0] @ want["ev"])
    if name == "square":
        assert r["edge"] == 0                                  # four equal areas: the lowest edge
        assert abs(got_u * got_v) == 0.0 and abs(got_u) + abs(got_v) == 1.0
    else:
        assert (got_u, got_v) == (ax[0] / np.hypot(*ax), ax[1] / np.hypot(*ax))
        assert abs(np.arctan2(got_v, got_u) - np.arctan2(ax[1], ax[0])) <= 1e-15
    assert np.array_equal(P[:3, 1], np.cross(P[:3, 2], P[:3, 0]))


def test_planes_of_every_dominant_axis_and_sign_give_the_same_box():
    ref = BF.box_fit(*S.lattice_box(**S.KNOWN["rect_345"])[:2])
    for name in ("d_negative", "axis_x", "axis_y"):
        r = BF.box_fit(*S.lattice_box(**S.KNOWN[name])[:2])
        assert np.array_equal(r["dims"], ref["dims"]) and (r["edge"], r["n_top"], r["rectangularity"]) == (ref["edge"], ref["n_top"], 1.0), name
    d = BF.box_fit(*S.lattice_box(**S.KNOWN["d_negative"])[:2])
    assert np.array_equal(d["pose"], ref["pose"])            # (the coefficients negated: step 1 orients them back)


@pytest.mark.parametrize("name,status,n_top,vertices,overflow", [
    ("two_points", BF.CD_ERR_FEW_CORRESPONDENCES, 0, 0, 0), ("nan_coordinate", BF.CD_ERR_INVALID_ARG, 0, 0, 0), ("beyond_range", BF.CD_ERR_INVALID_ARG, 0, 0, 0),
    ("no_plane", BF.CD_ERR_NO_MODEL, 0, 0, 0), ("top_collinear", BF.CD_ERR_NO_MODEL, 40, 2, 0), ("top_one_point", BF.CD_ERR_NO_MODEL, 20, 1, 0),
    ("stray_63", BF.CD_ERR_NO_MODEL, 1, 1, 0), ("parabola_overflow", BF.CD_ERR_CAPACITY, BF.MAX_HULL + 1, 0, 1)])
def test_every_status_holds_the_counts_and_zeros(name, status, n_top, vertices, overflow):
    r = fit(name)
    assert (r["status"], r["n"], r["n_top"], r["hull_vertices"], r["overflow"], r["edge"], r["match_slot"]) == \
        (status, len(S.kernel_cases()[name][1]), n_top, vertices, overflow, 0, -1)
    assert r["height_ref"] == 0 and not r["dims"].any() and not r["pose"].any() and r["area"] == 0 and r["rectangularity"] == 0 and r["match_cost"] == 0


def test_a_frame_without_a_plane_and_bad_bands():
    co, xyz, band = S.kernel_cases()["hull_4"]
    assert BF.box_fit(co, xyz, band, have_plane=False)["status"] == BF.CD_ERR_NO_MODEL
    assert BF.box_fit(np.array([0, 0, np.nan, 1], np.float32), xyz, band)["status"] == BF.CD_ERR_NO_MODEL
    for bad in (0.0, -1.0, np.nan, np.inf, 64.5):
        with pytest.raises(ValueError):
            BF.box_fit(co, xyz, bad)


def test_one_stray_high_point_does_not_set_the_level_from_64_points_on():
    assert fit("stray_64")["status"] == BF.CD_OK and fit("stray_64")["n_top"] == 64 and abs(fit("stray_64")["height_ref"] - 4000 / 65536.0) < 21 / 65536.0
    assert fit("stray_63")["n_top"] == 1                      # k = 1: the stray point is the level, and the only point in its band


def test_the_band_includes_its_lower_end():
    r = fit("on_the_band")
    assert (r["status"], r["n_top"], r["hull_vertices"]) == (BF.CD_OK, 5, 4)


def test_the_hull_cap_and_the_circle():
    assert (fit("parabola_max_hull")["status"], fit("parabola_max_hull")["hull_vertices"]) == (BF.CD_OK, BF.MAX_HULL)
    assert fit("circle")["hull_vertices"] == 656 and 0.75 < fit("circle")["rectangularity"] < 0.8       # pi / 4


# ---- cd_box_fit_match's rule ---------------------------------------------------------------------------------------------------------
def test_match_rule():
    assert BF.match([0.2, 0.1, 0.03], CONFIG5, 31, CONFIG5_TOLERANCE) == (0, 0.0)
    assert BF.match([0.1, 0.1, 0.1], CONFIG5, 31, CONFIG5_TOLERANCE) == (4, 0.0)
    assert BF.match([0.2, 0.1, 0.03], CONFIG5, 30, CONFIG5_TOLERANCE)[0] == -1                     # its slot not loaded: the next is 0.045 away
    assert BF.match([0.2, 0.1, 0.03], CONFIG5, 0, CONFIG5_TOLERANCE) == (-1, 0.0)
    assert BF.match([0.2, 0.1, 0.03], [[0.1, 0.2, 0.03]], 1, 0.0) == (0, 0.0)                      # a slot's first two are sorted
    tie = [[0.2, 0.1, 0.75], [0.2, 0.1, 0.25], [0.2, 0.1, 0.75]]                                    # (binary fractions: the costs are equal exactly)
    assert BF.match([0.2, 0.1, 0.5], tie, 7, 0.5) == (0, 0.25) and BF.match([0.2, 0.1, 0.5], tie, 6, 0.5) == (1, 0.25)     # a tie: the lowest slot
    s, c = BF.match([0.2, 0.1, 0.03], CONFIG5, 31, 1e-6)
    assert (s, c) == (0, 0.0)
    s, c = BF.match([0.2, 0.1005, 0.03], CONFIG5, 31, 1e-6)
    assert s == -1 and abs(c - 0.0005) < 1e-12


# ---- preconditions against the truth -------------------------------------------------------------------------------------------------
def test_synth_clusters_against_truth():
    """Frames 0..31 at default parameters, the oracle's clusters: |dL|, |dW| <= 3 leaves (two for the voxel centroids that locate the
    two sides, one for the depth noise that leans the visible side face into the band), |dH| <= leaf / 2, the centre within one leaf,
    the yaw within 3 degrees."""
    cl = S.synth_clusters(0, 32)
    assert len(cl) >= 32
    E = []
    for plane, pts, T, dims, _ in cl:
        r = BF.box_fit(plane, pts)
        assert r["status"] == BF.CD_OK
        E.append(S.errors(r, T, dims))
    E = np.abs(np.array(E))
    print("worst |dL| %.2f mm, |dW| %.2f mm, |dH| %.2f mm, centre %.2f mm, yaw %.2f deg" % (1e3 * E[:, 0].max(), 1e3 * E[:, 1].max(), 1e3 * E[:, 2].max(),
                                                                                     1e3 * E[:, 3].max(), E[:, 4].max()))
    assert E[:, 0].max() <= 3 * LEAF and E[:, 1].max() <= 3 * LEAF
    assert E[:, 2].max() <= LEAF / 2 and E[:, 3].max() <= LEAF and E[:, 4].max() <= 3.0


def test_config5_scenes_name_the_true_slot():
    """Config-5 scenes 0..7 at 640 x 480: the match rule with tolerance 0.0125 names the true slot of every cluster."""
    cl = S.config5_clusters(0, 8)
    assert len(cl) == 40
    worst = 0.0
    for plane, pts, _, _, b in cl:
        r = BF.box_fit(plane, pts)
        assert r["status"] == BF.CD_OK
        slot, cost = BF.match(r["dims"], CONFIG5, 31, CONFIG5_TOLERANCE)
        assert slot == b, (slot, b, cost)
        worst = max(worst, cost)
    print("worst true-slot cost %.2f mm" % (1e3 * worst))


# ---- the host arithmetic against the module -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["", "-fsanitize=address,undefined"], ids=["plain", "sanitized"])
def check_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("box_fit") / "box_fit_math_check")
    cmd = ["g++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
           "-Wno-unknown-pragmas"] + ([request.param, "-fno-sanitize-recover=all"] if request.param else []) + [os.path.join(CSRC, "box_fit_math_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def _write_sets(path, sets, mask=31, tol=CONFIG5_TOLERANCE):
    sd = np.zeros((capi.CD_MAX_TEMPLATES, 3), np.float64)
    sd[:5] = CONFIG5
    with open(path, "wb") as fp:
        fp.write(struct.pack("<i", len(sets)))
        for co, xyz, band, have in sets:
            p = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
            fp.write(struct.pack("<ii", len(p), int(have)) + np.asarray(co, np.float32).tobytes() + struct.pack("<dIId", band, mask, 0, tol) + sd.tobytes() + p.tobytes())


def _run_check(exe, tmp_path, sets):
    path = str(tmp_path / "sets.bin")
    _write_sets(path, sets)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.rstrip("\n").split("\n")
    assert len(lines) == 2 * len(sets)
    out = []
    for k in range(len(sets)):
        w = lines[2 * k].split()
        assert w[0] == "rec" and len(w) == 1 + 7 + 23
        m = lines[2 * k + 1].split()
        out.append((tuple(int(v) for v in w[1:8]) + tuple(int(v, 16) for v in w[8:]), (int(m[1]), int(m[2], 16))))
    return out


def _module_side(sets):
    out = []
    for co, xyz, band, have in sets:
        r = BF.box_fit(co, xyz, band, have_plane=bool(have))
        s, c = BF.match(r["dims"], CONFIG5, 31, CONFIG5_TOLERANCE)
        out.append((BF.record_bits(r), (s, int(np.float64(c).view(np.uint64)))))
    return out


def test_box_fit_math_on_the_kernel_cases(check_exe, tmp_path):
    names = sorted(S.kernel_cases())
    sets = [S.kernel_cases()[k] + (1,) for k in names] + [S.kernel_cases()["hull_4"] + (0,)]
    got, want = _run_check(check_exe, tmp_path, sets), _module_side(sets)
    for k, name in enumerate(names + ["frame_without_plane"]):
        assert got[k] == want[k], name


def test_box_fit_math_on_the_oracle_clusters_and_random_clouds(check_exe, tmp_path):
    sets = [(plane, pts, BF.BAND_DEFAULT, 1) for plane, pts, _, _, _ in S.synth_clusters(0, 32) + S.config5_clusters(0, 8)]
    sets += [S.random_cloud(seed, 50 + 37 * seed) + (0.004 + 0.001 * (seed % 5), 1) for seed in range(10, 40)]
    got, want = _run_check(check_exe, tmp_path, sets), _module_side(sets)
    assert sum(w[0][4] == BF.CD_OK for w in want) >= len(sets) - 2
    for k in range(len(sets)):
        assert got[k] == want[k], k


def test_check_program_refuses_bad_input(check_exe, tmp_path):
    path = str(tmp_path / "bad.bin")
    co, xyz, _ = S.kernel_cases()["hull_4"]
    _write_sets(path, [(co, xyz, -1.0, 1)])
    assert subprocess.run([check_exe, path], capture_output=True).returncode == 2
    with open(path, "wb") as fp:
        fp.write(struct.pack("<i", 1) + b"\0" * 10)
    assert subprocess.run([check_exe, path], capture_output=True).returncode == 2


def test_library_host_calls_equal_the_module():
    for name, (co, xyz, band) in sorted(S.kernel_cases().items()):
        want = BF.box_fit(co, xyz, band)
        assert S.same_record(capi.box_fit_host(co, xyz, band), want) == [], name
    for dims, mask, tol in (([0.2, 0.1, 0.03], 31, 0.0125), ([0.197, 0.108, 0.031], 31, 0.0125), ([0.2, 0.1, 0.03], 30, 0.0125), ([0.15, 0.149, 0.06], 31, 1e-6),
                            ([0.2, 0.1, 0.03], 0, 1.0)):
        assert capi.box_fit_match(dims, CONFIG5, mask, tol) == BF.match(dims, CONFIG5, mask, tol)
    lib = capi.load_library()
    co, xyz, band = S.kernel_cases()["hull_4"]
    p = np.ascontiguousarray(xyz)
    out = capi.CdBoxFit()
    for args in ((None, capi._ptr(p), 12, len(p), band, C.byref(out)), (capi._ptr(co), None, 12, len(p), band, C.byref(out)),
                 (capi._ptr(co), capi._ptr(p), 8, len(p), band, C.byref(out)), (capi._ptr(co), capi._ptr(p), 12, -1, band, C.byref(out)),
                 (capi._ptr(co), capi._ptr(p), 12, len(p), 0.0, C.byref(out)), (capi._ptr(co), capi._ptr(p), 12, len(p), float("nan"), C.byref(out)),
                 (capi._ptr(co), capi._ptr(p), 12, len(p), band, None)):
        assert lib.cd_box_fit_host(*args) == capi.CD_ERR_INVALID_ARG
