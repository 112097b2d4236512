"""The two-way registration score (rule C21) on the CPU: the numpy specification (perception_amd/pair_score.py) on hand-made known
answers and against a float64 k-d tree, the host arithmetic of pair_score_math.hpp (pair_score_math_check, plain and sanitized;
cd_pair_score_host) against the module in every field, bit for bit, the validation of the thresholds and the names the header and
capi.py export."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

from conftest import GOLDEN, ROOT
from perception_amd import capi, pair_score as PS, pcd

CSRC = os.path.join(ROOT, "perception_amd", "csrc")
NEW_SYMBOLS = ["cd_set_pair_score", "cd_get_pair_score", "cd_pair_score_struct_size", "cd_get_cluster_pair_scores", "cd_pair_score_points",
               "cd_pair_score_host"]
f32 = np.float32
IDENT = np.eye(4, dtype=f32)


def bits(v):
    return int(np.float64(v).view(np.uint64))


def same_record(a, b):
    """Every field: the integers equal, the doubles equal in their bits."""
    for k in PS.FIELDS:
        if isinstance(a[k], float) or isinstance(b[k], float):
            assert bits(a[k]) == bits(b[k]), (k, a[k], b[k])
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def small_motion(angle_deg=3.0, shift=(0.002, -0.001, 0.0015)):
    a = np.deg2rad(angle_deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = shift
    return T.astype(f32)


def test_header_and_capi_export_the_names():
    header = open(os.path.join(ROOT, "include", "cuboid_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS
    assert C.sizeof(capi.CdPairScore) == 64 and capi.load_library().cd_pair_score_struct_size() == 64      # 6 int32, 5 doubles, no hole
    assert [n for n, _ in capi.CdPairScore._fields_] == list(PS.FIELDS)
    for m in ("set_pair_score", "pair_score_setting", "cluster_pair_scores", "pair_score_points"):
        assert callable(getattr(capi.Context, m))
    for name, value in (("RANGE", capi.CD_PAIR_SCORE_RANGE_DEFAULT), ("MIN_COVERAGE", capi.CD_PAIR_SCORE_MIN_COVERAGE_DEFAULT),
                        ("MIN_INLIER", capi.CD_PAIR_SCORE_MIN_INLIER_DEFAULT)):
        assert float(re.search(r"#define\s+CD_PAIR_SCORE_%s_DEFAULT\s+([0-9.]+)" % name, header).group(1)) == value


# ---- the specification on known answers -------------------------------------------------------------------------------------------
def test_two_template_points_and_a_distance_equal_to_tau():
    """f = 0, 1/16, 1/4 and r = 0, 1/16; the range 1/4 has tau = 1/16 exactly, and the distances equal to it are inside."""
    src = np.array([[0, 0, 0], [1, 0, 0], [0, 0.5, 0]], f32)
    tpl = np.array([[0, 0, 0], [1, 0, 0.25]], f32)
    assert PS.tau_of(0.25) == f32(0.0625)
    o = PS.pair_score(src, IDENT, tpl, 0.25, 1.0, 2.0 / 3.0, 1, want_distances=True)
    assert o["f"].tolist() == [0.0, 0.0625, 0.25] and o["r"].tolist() == [0.0, 0.0625]
    assert (o["n_source"], o["n_source_in"], o["n_template"], o["n_template_in"], o["status"]) == (3, 2, 2, 2, 0)
    assert (o["forward_fitness_in"], o["reverse_fitness_in"], o["reverse_fitness"]) == (0.03125, 0.03125, 0.03125)
    assert (o["coverage"], o["inlier_fraction"]) == (1.0, 2.0 / 3.0)
    assert o["valid"] == 1                                            # both fractions on their boundary: valid
    assert PS.pair_score(src, IDENT, tpl, 0.25, 1.0, np.nextafter(2.0 / 3.0, 1.0), 1)["valid"] == 0
    assert PS.pair_score(src, IDENT, tpl, 0.25, 1.0, 2.0 / 3.0, 0)["valid"] == 0      # accepted is the result's own flag
    # one float below the distance: outside
    below = float(np.sqrt(np.float64(np.nextafter(f32(0.0625), f32(0)))))
    assert PS.tau_of(below) < f32(0.0625)
    assert PS.pair_score(src, IDENT, tpl, below, 0, 0, 1)["n_source_in"] == 1


def test_a_point_at_the_range_in_double_but_above_tau_in_float():
    """A point whose distance is exactly d as a double, and whose float32 squared distance rounds up past d * d: outside."""
    found = 0
    for k in range(1, 60):
        x = f32(0.1) + f32(k) * f32(2.0 ** -10)
        d = float(x)                                                  # the point's distance, exactly
        d2 = x * x                                                    # float32
        if np.float64(d2) > np.float64(d) * np.float64(d):
            src = np.array([[x, 0, 0], [0, 0, 0], [0, 0, 0]], f32)
            o = PS.pair_score(src, IDENT, np.zeros((1, 3), f32), d, 0, 0, 1, want_distances=True)
            assert o["f"][0] == d2 and d2 > PS.tau_of(d) and o["n_source_in"] == 2 and o["n_template_in"] == 1
            found += 1
    assert found >= 5


def test_three_source_points_and_one_template_point():
    src = np.array([[0.5, 0, 0], [0, 0.25, 0], [0, 0, 2]], f32)
    o = PS.pair_score(src, IDENT, np.zeros((1, 3), f32), 1.0, 0, 0, 1)
    assert (o["n_source_in"], o["n_template_in"], o["status"]) == (2, 1, 0)
    assert (o["forward_fitness_in"], o["reverse_fitness_in"], o["reverse_fitness"]) == ((0.25 + 0.0625) / 2, 0.0625, 0.0625)
    assert (o["coverage"], o["inlier_fraction"]) == (1.0, 2.0 / 3.0)


def test_identical_sets():
    p = np.random.default_rng(3).uniform(-0.1, 0.1, (200, 3)).astype(f32)
    o = PS.pair_score(p, IDENT, p[::-1], 0.001, 1.0, 1.0, 1)
    assert (o["coverage"], o["inlier_fraction"], o["valid"]) == (1.0, 1.0, 1)
    assert (o["forward_fitness_in"], o["reverse_fitness_in"], o["reverse_fitness"]) == (0.0, 0.0, 0.0)


def test_the_single_evaluation_of_T():
    """Step 1's order, one rounding per operation (a fused multiply-add would give other bits for these values)."""
    T = small_motion(7.0)
    p = np.random.default_rng(4).uniform(-0.3, 0.3, (500, 3)).astype(f32)
    A = PS.aligned(T, p)
    for i in (0, 17, 499):
        x, y, z = p[i]
        want = [f32(f32(f32(f32(T[r, 0] * x) + f32(T[r, 1] * y)) + f32(T[r, 2] * z)) + T[r, 3]) for r in range(3)]
        assert A[i].tolist() == want


def test_terms_are_clamped_and_nothing_overflows():
    """A source 100 m from the template: every r is 10^4, its term 256; the inside sums are empty."""
    src = np.array([[100, 0, 0], [100, 0, 0], [100, 0, 0]], f32)
    tpl = np.zeros((5, 3), f32)
    o = PS.pair_score(src, IDENT, tpl, 0.01, 0, 0, 1)
    assert (o["n_source_in"], o["n_template_in"], o["reverse_fitness"], o["forward_fitness_in"], o["reverse_fitness_in"]) == (0, 0, 256.0, 0.0, 0.0)
    assert PS.fix_sum(np.full(1 << 19, np.inf, f32)[:4]) == 4 << 44 and (1 << 19) * (1 << 44) == 1 << 63      # the bound of step 5
    o = PS.pair_score(src, IDENT, tpl, 1000.0, 0, 0, 1)               # a range beyond the clamp: inside, the term still 256
    assert (o["n_source_in"], o["forward_fitness_in"]) == (3, 256.0)


def test_statuses():
    p = np.random.default_rng(5).uniform(-0.1, 0.1, (10, 3)).astype(f32)
    zero = dict(PS._record(0, 0, 0))
    cases = [(p, IDENT, np.zeros((0, 3), f32), PS.CD_ERR_NO_TEMPLATE), (p[:2], IDENT, np.zeros((0, 3), f32), PS.CD_ERR_NO_TEMPLATE),
             (p[:2], IDENT, p, PS.CD_ERR_FEW_CORRESPONDENCES), (p[:0], IDENT, p, PS.CD_ERR_FEW_CORRESPONDENCES)]
    Tn = IDENT.copy(); Tn[1, 2] = np.nan
    Ti = IDENT.copy(); Ti[3, 0] = np.inf                              # (the bottom row is read by nothing but the check)
    big = IDENT.copy(); big[0, 0] = f32(3e38)
    q = p.copy(); q[4, 1] = np.inf
    cases += [(p, Tn, p, PS.CD_ERR_INVALID_ARG), (p, Ti, p, PS.CD_ERR_INVALID_ARG), (p, IDENT, q, PS.CD_ERR_INVALID_ARG), (q, IDENT, p, PS.CD_ERR_INVALID_ARG),
              (p * f32(1e3), big, p, PS.CD_ERR_INVALID_ARG),           # A overflows
              (np.zeros((PS.MAX_POINTS + 1, 3), f32), IDENT, p[:1], PS.CD_ERR_CAPACITY)]
    for src, T, tpl, status in cases:
        o = PS.pair_score(src, T, tpl, 0.01, 0, 0, 1)
        assert o == dict(zero, n_source=len(src), n_template=len(tpl), status=status)
    for bad in ((0.0, 0, 0), (-1.0, 0, 0), (np.nan, 0, 0), (np.inf, 0, 0), (0.01, -0.1, 0), (0.01, 0, 1.5), (0.01, np.nan, 0)):
        assert not PS.check_thresholds(*bad)
        with pytest.raises(ValueError):
            PS.pair_score(p, IDENT, p, *bad)
    assert PS.check_thresholds(1e-9, 0.0, 1.0)


@pytest.mark.parametrize("n,m,seed", [(700, 900, 1), (300, 2000, 2), (1500, 400, 3)])
def test_against_a_float64_kd_tree(n, m, seed):
    """Wherever no float64 squared distance is within 1e-6 relative of tau, the inside flags - and so the counts - agree with an exact
    float64 nearest-neighbour search over the same aligned points."""
    rng = np.random.default_rng(seed)
    tpl = rng.uniform(-0.1, 0.1, (m, 3)).astype(f32)
    src = (tpl[rng.choice(m, n, replace=n > m)] + rng.normal(scale=0.004, size=(n, 3))).astype(f32)
    T = small_motion(2.0)
    d = 0.006
    o = PS.pair_score(src, T, tpl, d, 0, 0, 1, want_distances=True)
    A = PS.aligned(T, src).astype(np.float64)
    tau = np.float64(PS.tau_of(d))
    skipped = 0
    for mine, (q, t) in ((o["f"], (A, tpl.astype(np.float64))), (o["r"], (tpl.astype(np.float64), A))):
        d2 = cKDTree(t).query(q)[0] ** 2
        clear = np.abs(d2 - tau) > 1e-6 * tau
        skipped += int((~clear).sum())
        assert np.array_equal((mine <= f32(tau))[clear], (d2 <= tau)[clear])
        assert np.allclose(mine.astype(np.float64), d2, rtol=1e-4, atol=1e-12)
    assert skipped == 0                                               # nothing was left out of the comparison
    assert 0 < o["n_source_in"] < n and 0 < o["n_template_in"] < m    # the bound does bound


# ---- pair_score_math.hpp on the host ------------------------------------------------------------------------------------------------
def scanned(name):
    return np.ascontiguousarray(pcd.read_xyz(os.path.join(GOLDEN, name + "_ascii.pcd")).astype(f32))


def host_cases():
    rng = np.random.default_rng(9)
    box = lambda n: rng.uniform(-0.1, 0.1, (n, 3)).astype(f32)
    p = box(10)
    Tn = IDENT.copy(); Tn[0, 3] = np.nan
    q = p.copy(); q[3, 2] = -np.inf
    far = box(40) + f32(100.0)
    marker, clamp = scanned("marker"), scanned("clamp")
    return [("known", np.array([[0, 0, 0], [1, 0, 0], [0, 0.5, 0]], f32), IDENT, np.array([[0, 0, 0], [1, 0, 0.25]], f32), 0.25, 1.0, 2.0 / 3.0, 1),
            ("3x1", box(3), small_motion(), box(1), 0.05, 0.5, 0.5, 1), ("random", box(777), small_motion(), box(1300), 0.008, 0.3, 0.3, 1),
            ("not_accepted", box(100), small_motion(), box(90), 0.02, 0.0, 0.0, 0), ("ties", np.repeat(box(40), 3, axis=0), IDENT, np.repeat(box(30), 2, axis=0), 0.02, 0.2, 0.2, 1),
            ("far", far, IDENT, box(50), 0.01, 0.1, 0.1, 1), ("marker_on_clamp", marker[::2], small_motion(4.0), clamp, 0.005, 0.4, 0.5, 1),
            ("empty_slot", p, IDENT, np.zeros((0, 3), f32), 0.01, 0, 0, 1), ("two_points", p[:2], IDENT, p, 0.01, 0, 0, 1), ("nan_T", p, Tn, p, 0.01, 0, 0, 1),
            ("inf_template", p, IDENT, q, 0.01, 0, 0, 1), ("inf_source", q, IDENT, p, 0.01, 0, 0, 1)]


@pytest.fixture(scope="module", params=["", "-fsanitize=address,undefined"], ids=["plain", "sanitized"])
def check_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pair") / "pair_score_math_check")
    cmd = ["g++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
           "-Wno-unknown-pragmas"] + ([request.param] if request.param else []) + [os.path.join(CSRC, "pair_score_math_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def _run_check(exe, tmp_path, src, T, tpl, d, cov, inl, accepted):
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as fp:
        fp.write(struct.pack("<iiii", len(tpl), len(src), accepted, 0) + np.asarray(T, "<f4").tobytes() + struct.pack("<ddd", d, cov, inl))
        fp.write(np.ascontiguousarray(tpl, "<f4").tobytes() + np.ascontiguousarray(src, "<f4").tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(line.split(" ", 1) for line in r.stdout.rstrip("\n").split("\n"))
    rec = dict(zip(PS.FIELDS[:6], (int(v) for v in lines["counts"].split())))
    rec.update(zip(PS.FIELDS[6:], (float(np.uint64(int(v, 16)).view(np.float64)) for v in lines["values"].split())))
    return rec


@pytest.mark.parametrize("case", host_cases(), ids=[c[0] for c in host_cases()])
def test_pair_score_math_on_the_host(check_exe, tmp_path, case):
    _, src, T, tpl, d, cov, inl, accepted = case
    same_record(_run_check(check_exe, tmp_path, src, T, tpl, d, cov, inl, accepted), PS.pair_score(src, T, tpl, d, cov, inl, accepted))


def test_check_program_refuses_bad_thresholds(check_exe, tmp_path):
    path = str(tmp_path / "bad.bin")
    with open(path, "wb") as fp:
        fp.write(struct.pack("<iiii", 0, 0, 1, 0) + IDENT.tobytes() + struct.pack("<ddd", 0.0, 0.5, 0.5))
    assert subprocess.run([check_exe, path], capture_output=True).returncode == 2


@pytest.mark.parametrize("case", host_cases(), ids=[c[0] for c in host_cases()])
def test_library_host_call_equals_the_module(case):
    _, src, T, tpl, d, cov, inl, accepted = case
    same_record(capi.pair_score_host(tpl, src, T, d, cov, inl, accepted), PS.pair_score(src, T, tpl, d, cov, inl, accepted))


def test_library_host_call_with_strides_and_bad_arguments():
    lib = capi.load_library()
    rng = np.random.default_rng(12)
    src, tpl = rng.uniform(-0.1, 0.1, (50, 4)).astype(f32), rng.uniform(-0.1, 0.1, (60, 5)).astype(f32)
    T = np.ascontiguousarray(small_motion().ravel())
    out = capi.CdPairScore()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.cd_pair_score_host(vp(tpl), 20, 60, vp(src), 16, 50, vp(T), 0.02, 0.1, 0.1, 1, C.byref(out)) == capi.CD_OK
    same_record(out.as_dict(), PS.pair_score(src[:, :3], T, tpl[:, :3], 0.02, 0.1, 0.1, 1))
    # what the setter refuses, the calls refuse: a range that is not finite and > 0, a fraction outside [0, 1]
    for bad in ((0.0, 0.1, 0.1), (-0.01, 0.1, 0.1), (float("nan"), 0.1, 0.1), (float("inf"), 0.1, 0.1), (0.02, -0.1, 0.1), (0.02, 0.1, 1.0001), (0.02, float("nan"), 0.1)):
        assert lib.cd_pair_score_host(vp(tpl), 20, 60, vp(src), 16, 50, vp(T), bad[0], bad[1], bad[2], 1, C.byref(out)) == capi.CD_ERR_INVALID_ARG
    assert lib.cd_pair_score_host(vp(tpl), 20, 60, vp(src), 16, 50, vp(T), 0.02, 0.0, 1.0, 1, C.byref(out)) == capi.CD_OK
    assert lib.cd_pair_score_host(vp(tpl), 20, 60, vp(src), 16, 50, None, 0.02, 0.1, 0.1, 1, C.byref(out)) == capi.CD_ERR_INVALID_ARG
    assert lib.cd_pair_score_host(vp(tpl), 8, 60, vp(src), 16, 50, vp(T), 0.02, 0.1, 0.1, 1, C.byref(out)) == capi.CD_ERR_INVALID_ARG
    # a context-free setter and getter refuse a null context
    assert lib.cd_set_pair_score(None, 1, 0.01, 0.5, 0.5) == capi.CD_ERR_INVALID_ARG and lib.cd_get_cluster_pair_scores(None, 0, 0, 0, None) == capi.CD_ERR_INVALID_ARG
