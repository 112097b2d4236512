"""The table prism (rule C20) on the CPU: the numpy specification (perception_amd/table_prism.py) on known answers, the host
arithmetic of prism_math.hpp (prism_math_check, plain and sanitized; the library's two host helpers) against the module, and the
names the header and capi.py export."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import prism_scenarios as PS
from conftest import ROOT
from perception_amd import capi, table_prism as TP

CSRC = os.path.join(ROOT, "perception_amd", "csrc")
NEW_SYMBOLS = ["cd_set_table_prism", "cd_get_table_prism", "cd_prism_struct_size", "cd_get_prism_stats", "cd_get_prism_hull", "cd_table_prism",
               "cd_prism_project", "cd_prism_hull_host"]


def run(c):
    return TP.table_prism(c["plane"], c["coeff"], c["xyz"], *c["limits"])


def kept_uv(c, o):
    return [tuple(int(v) for v in uv) for uv in TP.project(c["coeff"], c["xyz"])[1][o["indices"]]]


def test_header_and_capi_export_the_names():
    header = open(os.path.join(ROOT, "include", "cuboid_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS
    assert (capi.CD_PRISM_MAX_HULL, capi.CD_PRISM_LDS_POINTS) == (TP.MAX_HULL, TP.LDS_POINTS)
    assert re.search(r"#define\s+CD_PRISM_MAX_HULL\s+%d\b" % TP.MAX_HULL, header) and re.search(r"#define\s+CD_PRISM_LDS_POINTS\s+%d\b" % TP.LDS_POINTS, header)
    assert C.sizeof(capi.CdPrismStats) == 48 and capi.load_library().cd_prism_struct_size() == 48
    for m in ("set_table_prism", "table_prism_setting", "prism_stats", "prism_hull", "table_prism"):
        assert callable(getattr(capi.Context, m))


# ---- the specification on known answers -------------------------------------------------------------------------------------------
def test_square_with_interior_points():
    cases = PS.small_cases()
    for name in ("square", "collinear_and_duplicates"):       # collinear triples and duplicates are dropped: the same four
        c = cases[name]
        o = run(c)
        assert [tuple(v) for v in o["hull"].tolist()] == PS.SQUARE, name
        # inside, on an edge, on a vertex: kept; one unit outside: not
        assert kept_uv(c, o) == [(5, 5), (5, 0), (10, 5), (10, 10), (0, 0), (0, 10), (3, 7)], name
        s = o["stats"]
        assert (s["n_before"], s["n_kept"], s["n_below"], s["n_above"], s["n_outside"], s["hull_vertices"], s["axis_u"], s["axis_v"], s["overflow"]) == \
            (10, 7, 0, 0, 3, 4, 0, 1, 0), name
        assert o["indices"].dtype == np.int32 and np.array_equal(o["height"], c["xyz"][:, 2].astype(np.float64))


@pytest.mark.parametrize("name,vertices", [("all_collinear", 2), ("no_inlier", 0), ("one_inlier", 1), ("two_inliers", 2), ("one_point_many_times", 1)])
def test_fewer_than_three_vertices_keep_nothing(name, vertices):
    c = PS.small_cases()[name]
    o = run(c)
    s = o["stats"]
    assert len(o["hull"]) == s["hull_vertices"] == vertices and len(o["indices"]) == s["n_kept"] == 0
    assert s["n_outside"] == s["n_before"] == len(c["xyz"]) and s["overflow"] == 0
    if name == "all_collinear":
        assert o["hull"].tolist() == [[-5, -10], [8, 16]]


def test_triangle_hull_starts_at_the_smallest_point_and_runs_counter_clockwise():
    c = PS.small_cases()["triangle"]
    o = run(c)
    assert o["hull"].tolist() == [[0, 0], [7, 1], [3, 9]]
    assert kept_uv(c, o) == [(5, 5), (0, 0), (3, 7), (3, 3), (7, 1), (5, 5), (2, 6)]   # (2, 6) is on the edge (3, 9) -> (0, 0)


def test_points_on_edges_and_vertices_are_kept():
    c = PS.edge_case()
    o = run(c)
    assert o["hull"].tolist() == [[0, 0], [12, 4], [16, 16], [4, 12]]
    assert o["indices"].tolist() == list(range(15)) and o["stats"]["n_outside"] == 9


def test_height_limits_are_inclusive():
    c = PS.small_cases()["heights"]
    o = run(c)
    # z: 0, 0.02 (= min), 0.05 (= max), just below min, just above max, -0.01, 0.3, NaN, 0.03, 0.04
    assert o["indices"].tolist() == [1, 2, 8, 9]
    s = o["stats"]
    assert (s["n_below"], s["n_above"], s["n_outside"], s["n_kept"]) == (3, 3, 0, 4)          # the NaN height counts as above
    one = TP.table_prism(c["plane"], c["coeff"], c["xyz"], c["limits"][0], c["limits"][0])     # min == max: that height alone
    assert one["indices"].tolist() == [1]
    for bad in ((0.1, 0.0), (np.nan, 1.0), (0.0, np.inf)):
        with pytest.raises(ValueError):
            TP.table_prism(c["plane"], c["coeff"], c["xyz"], *bad)


def test_coeff_and_its_negative_give_identical_outputs():
    rng = np.random.RandomState(3)
    nrm = np.array([0.05, -0.75, -0.66])
    nrm /= np.linalg.norm(nrm)
    coeff = np.r_[nrm, 0.42].astype(np.float32)
    e1 = np.cross(nrm, [0, 0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    p0 = -0.42 * nrm
    plane = (p0 + rng.uniform(-0.2, 0.2, (400, 1)) * e1 + rng.uniform(-0.3, 0.3, (400, 1)) * e2 + rng.normal(0, 0.002, (400, 1)) * nrm).astype(np.float32)
    xyz = (p0 + rng.uniform(-0.3, 0.3, (300, 1)) * e1 + rng.uniform(-0.4, 0.4, (300, 1)) * e2 + rng.uniform(-0.05, 0.1, (300, 1)) * nrm).astype(np.float32)
    a = TP.table_prism(plane, coeff, xyz, 0.0, 0.05)
    b = TP.table_prism(plane, -coeff, xyz, 0.0, 0.05)
    assert a["stats"] == b["stats"] and np.array_equal(a["indices"], b["indices"]) and np.array_equal(a["hull"], b["hull"])
    assert np.array_equal(a["height"].view(np.uint64), b["height"].view(np.uint64))
    s = a["stats"]
    assert min(s["n_kept"], s["n_below"], s["n_above"], s["n_outside"]) > 0 and s["hull_vertices"] >= 3
    # the sensor at the origin is on the positive side, whichever sign the coefficients come with
    assert TP.project(coeff, np.zeros((1, 3), np.float32))[0][0] == TP.project(-coeff, np.zeros((1, 3), np.float32))[0][0] == np.float64(np.float32(0.42))


@pytest.mark.parametrize("abc,axes", [((1, 0.5, 0.5), (1, 2)), ((0.5, 1, 0.5), (0, 2)), ((0.5, 0.5, 1), (0, 1)), ((1, 1, 1), (1, 2)), ((0.5, 1, 1), (0, 2)),
                                      ((1, 0.5, 1), (1, 2)), ((-1, 1, 0.5), (1, 2)), ((0.5, -1, 1), (0, 2)), ((0.2, 0.3, -0.9), (0, 1))])
def test_tie_rule_of_the_dropped_axis(abc, axes):
    coeff = np.array(list(abc) + [0.3], np.float32)
    assert TP.axes(coeff) == axes
    assert TP.project(coeff, np.ones((1, 3), np.float32))[2] == axes
    o = TP.table_prism(np.zeros((0, 3), np.float32), coeff, np.ones((1, 3), np.float32), 0.0, 1.0)
    assert (o["stats"]["axis_u"], o["stats"]["axis_v"]) == axes


def test_quantisation_floors_and_clamps():
    p = np.array([[-0.5 / 65536, 1.25 / 65536, 0], [1e9, -1e9, 0], [np.nan, np.inf, 0], [8191.999, -8192.0, 0]], np.float32)
    _, uv, _ = TP.project(PS.COEFF_Z, p)
    assert uv.tolist() == [[-1, 1], [TP.QMAX, TP.QMIN], [TP.QMIN, TP.QMIN], [int(np.floor(np.float64(np.float32(8191.999)) * 65536)), TP.QMIN]]


def test_parabola_at_the_cap_and_beyond():
    c = PS.parabola_case(1024)
    o = run(c)
    i = np.arange(1024)
    assert o["stats"]["hull_vertices"] == 1024 and o["stats"]["overflow"] == 0 and np.array_equal(o["hull"], np.stack([i, i * i], 1))
    # between the parabola and its chord, on two vertices, on the vertex (100, 10000); not (-1, 0) nor (100, 9999) one unit below it
    assert kept_uv(c, o) == [(10, 200), (500, 300000), (0, 0), (1023, 1023 ** 2), (100, 10000)]
    c = PS.parabola_case(1025)
    o = run(c)
    s = o["stats"]
    assert (s["overflow"], s["hull_vertices"], s["n_kept"], s["n_outside"]) == (1, 0, 0, 7) and len(o["hull"]) == 0 and len(o["indices"]) == 0


def test_frame_without_a_plane_passes_untouched():
    c = PS.small_cases()["square"]
    o = TP.table_prism(c["plane"], c["coeff"], c["xyz"], 0.0, 0.5, have_plane=False)
    assert o["indices"].tolist() == list(range(10)) and o["stats"] == dict(dict.fromkeys(TP.STAT_FIELDS, 0), n_before=10, n_kept=10)


def test_pruning_keeps_every_hull_vertex():
    for c in (PS.grid_case(500, 1), PS.wide_grid_case(20000, 2), PS.circle_case(), PS.parabola_case(300), PS.small_cases()["one_point_many_times"]):
        _, uv, _ = TP.project(c["coeff"], c["plane"])
        keep = TP.prune_survivors(uv)
        assert np.array_equal(TP.hull(uv[keep]), TP.hull(uv))
    _, uv, _ = TP.project(PS.COEFF_Z, PS.wide_grid_case(20000, 2)["plane"])
    assert TP.prune_survivors(uv).sum() < 2000                  # the pruning does prune
    _, uv, _ = TP.project(PS.COEFF_Z, PS.circle_case()["plane"])
    assert TP.prune_survivors(uv).sum() > TP.LDS_POINTS        # and a circle defeats it: the kernel's global-memory march


# ---- prism_math.hpp on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["", "-fsanitize=address,undefined"], ids=["plain", "sanitized"])
def check_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prism") / "prism_math_check")
    cmd = ["g++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
           "-Wno-unknown-pragmas"] + ([request.param] if request.param else []) + [os.path.join(CSRC, "prism_math_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def _run_check(exe, tmp_path, c):
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as fp:
        fp.write(struct.pack("<ii", len(c["plane"]), len(c["xyz"])) + np.asarray(c["coeff"], "<f4").tobytes() + struct.pack("<dd", *c["limits"]))
        fp.write(np.ascontiguousarray(c["plane"][:, :3], "<f4").tobytes() + np.ascontiguousarray(c["xyz"][:, :3], "<f4").tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict((line.split(" ", 1) + [""])[:2] for line in r.stdout.rstrip("\n").split("\n"))
    stats = dict(zip(TP.STAT_FIELDS, (int(v) for v in lines["stats"].split())))
    hull = np.array([int(v) for v in lines["hull"].split()], np.int32).reshape(-1, 2)
    height = np.array([int(v, 16) for v in lines["height"].split()], np.uint64)
    kept = np.array([ch == "1" for ch in lines["kept"].strip()], bool)
    return stats, hull, height, kept


def tilted_case():
    rng = np.random.RandomState(11)
    c = PS.wide_grid_case(3000, 4)
    coeff = np.array([0.1, -0.7, -0.7, 0.5], np.float32)
    plane = (rng.uniform(-0.5, 0.5, (3000, 3)) + [0, 0.3, 0.4]).astype(np.float32)
    xyz = (rng.uniform(-0.6, 0.6, (1500, 3)) + [0, 0.3, 0.4]).astype(np.float32)
    xyz[7] = np.nan
    return dict(plane=plane, coeff=coeff, xyz=xyz, limits=(-0.1, 0.2), _=c)


CHECK_CASES = [(k, (lambda k=k: PS.small_cases()[k])) for k in sorted(PS.small_cases())] + [
    ("grid_500_on_8x8", lambda: PS.grid_case(500, 1)), ("grid_65", lambda: PS.grid_case(65, 2)), ("grid_3_of_2x2", lambda: PS.grid_case(3, 3, span=2)),
    ("wide_grid_20000", lambda: PS.wide_grid_case(20000, 2)), ("circle", PS.circle_case), ("parabola_1024", lambda: PS.parabola_case(1024)),
    ("parabola_1025", lambda: PS.parabola_case(1025)), ("edges", PS.edge_case), ("tilted", tilted_case)]


@pytest.mark.parametrize("name,make", CHECK_CASES, ids=[c[0] for c in CHECK_CASES])
def test_prism_math_on_the_host(check_exe, tmp_path, name, make):
    c = make()
    o = run(c)
    stats, hull, height, kept = _run_check(check_exe, tmp_path, c)
    assert stats == o["stats"]
    assert np.array_equal(hull, o["hull"])
    assert np.array_equal(height, o["height"].view(np.uint64))
    assert np.array_equal(np.flatnonzero(kept), o["indices"])


def test_check_program_refuses_bad_arguments(check_exe, tmp_path):
    path = str(tmp_path / "bad.bin")
    with open(path, "wb") as fp:
        fp.write(struct.pack("<ii", 0, 0) + np.zeros(4, "<f4").tobytes() + struct.pack("<dd", 1.0, 0.0))
    assert subprocess.run([check_exe, path], capture_output=True).returncode == 2


def test_library_host_helpers_equal_the_module():
    c = tilted_case()
    h, uv, axes = TP.project(c["coeff"], c["xyz"])
    for i in (0, 1, 7, 500, 1499):
        gh, guv, gax = capi.prism_project(c["coeff"], c["xyz"][i])
        assert (np.float64(gh).view(np.uint64) == h[i].view(np.uint64)) and guv == tuple(uv[i]) and gax == axes
    for make in (lambda: PS.grid_case(500, 1), PS.circle_case, lambda: PS.parabola_case(1025), lambda: PS.small_cases()["all_collinear"],
                 lambda: PS.small_cases()["no_inlier"]):
        puv = TP.project(PS.COEFF_Z, make()["plane"])[1]
        assert np.array_equal(capi.prism_hull_host(puv), TP.hull(puv))
    lib = capi.load_library()
    puv = np.ascontiguousarray(TP.project(PS.COEFF_Z, PS.parabola_case(20)["plane"])[1])
    out, n = np.zeros((4, 2), np.int32), C.c_int()
    assert lib.cd_prism_hull_host(puv.ctypes.data_as(C.c_void_p), 20, out.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == capi.CD_ERR_CAPACITY and n.value == 20
    assert np.array_equal(out, puv[:4])
