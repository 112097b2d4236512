"""The pose information (rule C23) on the CPU: the numpy specification (perception_amd/pose_info.py) on known answers - one, two and
three exact faces, a third face growing point by point - against a float64 J^T J written from the definition and against
numpy's eigenvalues; the host arithmetic of pose_info_math.hpp (pose_info_math_check, plain and sanitized; cd_pose_info_host)
against the module in every field, bit for bit, on every scenario; the covariance in ROS order against central differences of the
published pose; every status; the refusals of the setting; the names the header and capi.py export."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pose_info_reference as PR
import pose_info_scenarios as S
from conftest import ROOT
from perception_amd import capi, pose_info as PI

CSRC = os.path.join(ROOT, "perception_amd", "csrc")
NEW_SYMBOLS = ["cd_set_pose_info", "cd_get_pose_info", "cd_pose_info_struct_size", "cd_get_cluster_pose_info", "cd_pose_info_points",
               "cd_pose_info_host", "cd_pose_info_ros_covariance"]
f32 = np.float32
IDENT = S.IDENT
CASES = S.cases()
IDS = [c[0] for c in CASES]


def bits(v):
    return int(np.float64(v).view(np.uint64))


def same_record(a, b):
    """Every field: the integers equal, the doubles equal in their bits."""
    for k in PI.INT_FIELDS:
        assert a[k] == b[k], (k, a[k], b[k])
    for k in PI.FLOAT_FIELDS:
        x, y = np.atleast_1d(np.asarray(a[k], np.float64)), np.atleast_1d(np.asarray(b[k], np.float64))
        assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)), (k, a[k], b[k])


def spec(case, **kw):
    _, src, T, tpl, d, support, accepted = case
    return PI.pose_info(src, T, tpl, d, support, accepted, **kw)


def test_header_and_capi_export_the_names():
    header = open(os.path.join(ROOT, "include", "cuboid_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS
    assert C.sizeof(capi.CdPoseInfo) == 744 and capi.load_library().cd_pose_info_struct_size() == 744      # 8 int32, 89 doubles, no hole
    assert [n for n, _ in capi.CdPoseInfo._fields_] == list(PI.FIELDS)
    for m in ("set_pose_info", "pose_info_setting", "cluster_pose_info", "pose_info_points"):
        assert callable(getattr(capi.Context, m))
    for name, value in (("RANGE", capi.CD_POSE_INFO_RANGE_DEFAULT), ("MIN_SUPPORT", capi.CD_POSE_INFO_MIN_SUPPORT_DEFAULT)):
        assert float(re.search(r"#define\s+CD_POSE_INFO_%s_DEFAULT\s+([0-9.]+)" % name, header).group(1)) == value
    assert (PI.RANGE_DEFAULT, PI.MIN_SUPPORT_DEFAULT) == (capi.CD_POSE_INFO_RANGE_DEFAULT, capi.CD_POSE_INFO_MIN_SUPPORT_DEFAULT)
    assert capi.CD_POSE_INFO_RANGE_DEFAULT == capi.CD_PAIR_SCORE_RANGE_DEFAULT
    s = capi.CD_POSE_INFO_MIN_SUPPORT_DEFAULT
    assert s > 0 and np.log2(s) == int(np.log2(s))                                                            # a power of two


# ---- the specification on known answers -------------------------------------------------------------------------------------------
def test_one_exact_face_leaves_three_twists_free():
    """Exact points of the face of constant z: the eigenvalues 0 - 2 are exactly 0.0; free are the two in-face translations and the
    rotation about the normal, in index order (rotation z, translation x, translation y)."""
    src, T, tpl = S.exact_one_face()
    assert S.faces_of("tpl3")[0][0] == 2
    o = PI.pose_info(src, T, tpl, S.RANGE, 1.0, 1)
    assert o["status"] == 0 and o["n_in"] == len(src) and o["n_face"] == [0, 0, len(src)]
    assert [bits(v) for v in o["eigenvalues"][:3]] == [0, 0, 0] and o["eigenvalues"][3] > 1.0
    assert (o["n_constrained"], o["well_posed"], o["sigma2"]) == (3, 0, 0.0)
    V = np.array(o["eigenvectors"]).reshape(6, 6)
    assert V[:3].tolist() == np.eye(6)[[2, 3, 4]].tolist() and o["weakest"] == V[0].tolist()
    assert o["eigenvalues"][5] == pytest.approx(len(src), rel=0.2)                          # the translation along the normal: every point
    assert np.array_equal(np.array(o["covariance"]), np.zeros(36))                          # exact points: no residual


def test_two_exact_faces_leave_the_common_edge_free():
    src, T, tpl = S.exact_two_faces()
    o = PI.pose_info(src, T, tpl, S.RANGE, 1.0, 1)
    assert o["n_face"][0] == 0 and o["n_face"][1] > 0 and o["n_face"][2] > 0
    assert abs(o["eigenvalues"][0]) < 1e-9 and (o["n_constrained"], o["well_posed"]) == (5, 0)
    assert np.abs(np.array(o["weakest"]) - np.eye(6)[3]).max() < 1e-9                       # the translation along x, the common edge


def test_three_faces_constrain_everything():
    src, T, tpl = S.exact_three_faces()
    o = PI.pose_info(src, T, tpl, S.RANGE, 1.0, 1)
    assert min(o["n_face"]) > 0 and (o["n_constrained"], o["well_posed"]) == (6, 1)
    assert PI.pose_info(src, T, tpl, S.RANGE, 1.0, 0)["well_posed"] == 0                    # accepted is the result's own flag
    assert PI.pose_info(src, T, tpl, S.RANGE, 1e6, 1)["n_constrained"] == 0


def test_a_third_face_constrains_by_its_points():
    """Two exact faces plus k exact points of the third: the least eigenvalue rises with k, and stays below k (a point is worth at
    most one point)."""
    lam = [PI.pose_info(*S.exact_two_faces_plus(k), S.RANGE, 1.0, 1)["eigenvalues"][0] for k in S.PLUS]
    print("lambda_0 for k =", S.PLUS, ":", lam)
    assert all(a < b for a, b in zip(lam[:-1], lam[1:])) and lam[0] > 1e-3
    assert all(l <= k for l, k in zip(lam, S.PLUS))


def test_noisy_views_by_faces_seen():
    got = {c[0]: spec(c) for c in CASES if c[0].startswith("view_")}
    print({k: (v["n_face"], ["%.3g" % x for x in v["eigenvalues"]]) for k, v in got.items()})
    assert got["view_three"]["n_constrained"] == 6 and got["view_three"]["well_posed"] == 1
    assert got["view_one"]["n_constrained"] < 6 and got["view_two"]["n_constrained"] < 6
    assert 0.5e-3 ** 2 < got["view_three"]["sigma2"] < 2e-3 ** 2                           # the noise along the normals: 1 mm
    assert got["view_three_few"]["eigenvalues"][5] < got["view_three"]["eigenvalues"][5]    # fewer points, less information


def test_tau_and_ties_and_the_far_points():
    o = PI.pose_info(*S.tau_case(), S.SUPPORT, 1)
    assert (o["n_in"], o["status"]) == (4, 0)                                               # the distance equal to tau is inside, a float more is not
    o = PI.pose_info(*S.far_case(), 1.0, 1)
    assert o["status"] == 0 and o["sigma2"] > 100.0                                         # the far points were kept
    src, T, tpl, d = S.tie_case()
    o = PI.pose_info(src, T, tpl, d, 1.0, 1)
    assert o["n_in"] == len(src) and o["status"] == 0


# ---- the matrix and its decomposition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_information_matrix_against_float64(case):
    """Every term of a sum carries at most three float32 roundings (two subtractions against c0, one product: 3 * 2^-24 of its
    magnitude) and one fixed-point rounding; |a term of H_ij| sums to at most sqrt(H_ii H_jj) <= trace.  So |H - J^T J| <= 2^-22
    trace, entry by entry."""
    o = spec(case, want_matrix=True)
    assert o["status"] == 0
    _, src, T, tpl, d, _, _ = case
    H, ref = np.array(o["H"]), PR.information_f64(src, T, tpl, d)
    err = np.abs(H - ref).max() / np.trace(ref)
    print(case[0], "max |H - J^T J| / trace = %.2e" % err)
    assert err <= 2.0 ** -22
    assert np.array_equal(H, H.T)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_jacobi_against_numpy(case):
    """The sweeps leave off-diagonal entries below 2^-44 trace (the rule's own bound on the sweep count); by Weyl's inequality
    such a remainder moves an eigenvalue by at most its norm, <= 5 * 2^-44 trace for a 6 x 6 matrix with a zero diagonal, and
    numpy's own eigenvalues are good to a few 2^-52 trace: the two agree to 6 * 2^-44 trace.  Vectors: orthonormal, H v = lambda v."""
    o = spec(case, want_matrix=True)
    assert o["status"] == 0
    H = np.array(o["H"])
    tr = np.trace(H)
    off = PI.jacobi(o["H"])[2]
    lam, V = np.array(o["eigenvalues"]), np.array(o["eigenvectors"]).reshape(6, 6)
    err = np.abs(lam - np.linalg.eigvalsh(H)).max()
    print(case[0], "off-diagonal left / trace = %.2e, eigenvalue error / trace = %.2e" % (off / tr, err / tr))
    assert off < 2.0 ** -44 * tr
    assert err <= 6 * 2.0 ** -44 * tr
    assert np.all(np.diff(lam) >= 0)
    assert np.abs(V @ V.T - np.eye(6)).max() < 1e-13 and np.abs(H @ V.T - V.T * lam[None, :]).max() < 1e-12 * tr
    assert all(row[np.argmax(np.abs(row))] > 0 for row in V)


def test_covariance_is_the_pseudo_inverse_over_the_constrained_directions():
    o = spec([c for c in CASES if c[0] == "view_three"][0], want_matrix=True)
    L = o["length"]
    D = np.diag([1 / L] * 3 + [1.0] * 3)
    want = o["sigma2"] * D @ np.linalg.inv(np.array(o["H"])) @ D
    assert np.allclose(np.array(o["covariance"]).reshape(6, 6), want, rtol=1e-9, atol=0)
    two = spec([c for c in CASES if c[0] == "view_two"][0])
    C_ = np.array(two["covariance"]).reshape(6, 6)
    assert two["n_constrained"] < 6 and np.linalg.matrix_rank(C_, tol=1e-18) == two["n_constrained"]


# ---- pose_info_math.hpp on the host --------------------------------------------------------------------------------------------------
def status_cases():
    src, T, tpl = S.size_case(65)[0], S.motion(), S.tpl_small()
    rng = np.random.default_rng(3)
    Tn = T.copy(); Tn[1, 2] = np.nan
    Ti = T.copy(); Ti[3, 0] = np.inf                                                        # (the bottom row is read by nothing but the check)
    big = IDENT.copy(); big[0, 0] = f32(3e38)
    q = src.copy(); q[4, 1] = np.inf
    scanned = rng.uniform(-0.1, 0.1, (200, 3)).astype(f32)
    return [("empty_slot", src, T, np.zeros((0, 3), f32), PI.CD_ERR_NO_TEMPLATE), ("empty_slot_no_points", src[:0], T, np.zeros((0, 3), f32), PI.CD_ERR_NO_TEMPLATE),
            ("not_a_lattice", src, T, scanned, PI.CD_ERR_INVALID_ARG), ("nan_T", src, Tn, tpl, PI.CD_ERR_INVALID_ARG), ("inf_T", src, Ti, tpl, PI.CD_ERR_INVALID_ARG),
            ("inf_source", q, T, tpl, PI.CD_ERR_INVALID_ARG), ("overflow", src * f32(1e3), big, tpl, PI.CD_ERR_INVALID_ARG),
            ("no_points", src[:0], T, tpl, PI.CD_ERR_FEW_CORRESPONDENCES), ("far_away", src + f32(1.0), T, tpl, PI.CD_ERR_FEW_CORRESPONDENCES),
            ("two_inside", np.concatenate([tpl[[5, 300]], src + f32(1.0)]), IDENT, tpl, PI.CD_ERR_FEW_CORRESPONDENCES)]


def test_statuses():
    for name, src, T, tpl, status in status_cases():
        o = PI.pose_info(src, T, tpl, S.RANGE, S.SUPPORT, 1)
        assert o["status"] == status, name
        zero = PI._record(len(src), status, o["n_in"], o["n_face"])
        assert o == zero and (status == PI.CD_ERR_FEW_CORRESPONDENCES or o["n_in"] == 0), name
    assert PI.pose_info(np.concatenate([S.tpl_small()[[5, 300]], S.size_case(65)[0] + f32(1.0)]), IDENT, S.tpl_small(), S.RANGE, S.SUPPORT, 1)["n_in"] == 2
    for bad in ((0.0, 1.0), (-1.0, 1.0), (np.nan, 1.0), (np.inf, 1.0), (0.01, 0.0), (0.01, -2.0), (0.01, np.nan), (0.01, np.inf)):
        assert not PI.check_setting(*bad)
        with pytest.raises(ValueError):
            PI.pose_info(S.tpl_small(), IDENT, S.tpl_small(), *bad)
    assert PI.check_setting(1e-9, 1e-9)


def test_more_points_than_the_rule_sums():
    """n above 2^19 with correspondences: CD_ERR_CAPACITY with the counts, on the host as in the module (a two-row strip of the
    small template's first face: a lattice of 50 points, so that the brute-force search stays small)."""
    tpl = S.tpl_small()
    strip = tpl[:50]
    assert PI.IP.face_axes(strip).tolist() == [2] * 50
    src = np.tile(strip[:4], ((PI.MAX_POINTS >> 2) + 1, 1))
    want = PI.pose_info(src, IDENT, strip, S.RANGE, S.SUPPORT, 1)
    assert (want["status"], want["n_in"], want["n_source"]) == (PI.CD_ERR_CAPACITY, len(src), PI.MAX_POINTS + 4)
    same_record(capi.pose_info_host(strip, src, IDENT, S.RANGE, S.SUPPORT, 1), want)


@pytest.fixture(scope="module", params=["", "-fsanitize=address,undefined"], ids=["plain", "sanitized"])
def check_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pose") / "pose_info_math_check")
    cmd = ["g++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
           "-Wno-unknown-pragmas"] + ([request.param] if request.param else []) + [os.path.join(CSRC, "pose_info_math_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def _run_check(exe, tmp_path, src, T, tpl, d, support, accepted):
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as fp:
        fp.write(struct.pack("<iiii", len(tpl), len(src), accepted, 0) + np.asarray(T, "<f4").tobytes() + struct.pack("<dd", d, support))
        fp.write(np.ascontiguousarray(tpl, "<f4").tobytes() + np.ascontiguousarray(src, "<f4").tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(line.split(" ", 1) for line in r.stdout.rstrip("\n").split("\n"))
    c = [int(v) for v in lines["counts"].split()]
    v = [float(np.uint64(int(x, 16)).view(np.float64)) for x in lines["values"].split()]
    return dict(n_source=c[0], n_in=c[1], n_face=c[2:5], n_constrained=c[5], well_posed=c[6], status=c[7], eigenvalues=v[:6], eigenvectors=v[6:42],
                weakest=v[42:48], sigma2=v[48], covariance=v[49:85], centre=v[85:88], length=v[88])


ALL = [c for c in CASES] + [(n, s, T, t, S.RANGE, S.SUPPORT, 1) for n, s, T, t, _ in status_cases()]


@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_pose_info_math_on_the_host(check_exe, tmp_path, case):
    _, src, T, tpl, d, support, accepted = case
    same_record(_run_check(check_exe, tmp_path, src, T, tpl, d, support, accepted), PI.pose_info(src, T, tpl, d, support, accepted))


def test_check_program_refuses_a_bad_setting(check_exe, tmp_path):
    path = str(tmp_path / "bad.bin")
    with open(path, "wb") as fp:
        fp.write(struct.pack("<iiii", 0, 0, 1, 0) + IDENT.tobytes() + struct.pack("<dd", 0.005, 0.0))
    assert subprocess.run([check_exe, path], capture_output=True).returncode == 2


@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_library_host_call_equals_the_module(case):
    _, src, T, tpl, d, support, accepted = case
    same_record(capi.pose_info_host(tpl, src, T, d, support, accepted), PI.pose_info(src, T, tpl, d, support, accepted))


def test_library_host_call_with_strides_and_bad_arguments():
    lib = capi.load_library()
    _, src3, T, tpl3, d, support, _ = [c for c in CASES if c[0] == "view_three_few"][0]
    src, tpl = np.zeros((len(src3), 4), f32), np.zeros((len(tpl3), 5), f32)
    src[:, :3], tpl[:, :3] = src3, tpl3
    T = np.ascontiguousarray(T.ravel())
    out = capi.CdPoseInfo()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.cd_pose_info_host(vp(tpl), 20, len(tpl), vp(src), 16, len(src), vp(T), d, support, 1, C.byref(out)) == capi.CD_OK
    same_record(out.as_dict(), PI.pose_info(src3, T, tpl3, d, support, 1))
    # what the setter refuses, the calls refuse
    for bad in ((0.0, 1.0), (-0.01, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (d, 0.0), (d, -1.0), (d, float("nan")), (d, float("inf"))):
        assert lib.cd_pose_info_host(vp(tpl), 20, len(tpl), vp(src), 16, len(src), vp(T), bad[0], bad[1], 1, C.byref(out)) == capi.CD_ERR_INVALID_ARG
    assert lib.cd_pose_info_host(vp(tpl), 20, len(tpl), vp(src), 16, len(src), None, d, support, 1, C.byref(out)) == capi.CD_ERR_INVALID_ARG
    assert lib.cd_pose_info_host(vp(tpl), 8, len(tpl), vp(src), 16, len(src), vp(T), d, support, 1, C.byref(out)) == capi.CD_ERR_INVALID_ARG
    # the setter, the getter and the read-back refuse a null context
    assert lib.cd_set_pose_info(None, 1, 0.005, 16.0) == capi.CD_ERR_INVALID_ARG and lib.cd_get_pose_info(None, None, None, None) == capi.CD_ERR_INVALID_ARG
    assert lib.cd_get_cluster_pose_info(None, 0, 0, 0, None) == capi.CD_ERR_INVALID_ARG
    assert lib.cd_pose_info_ros_covariance(None, vp(T), vp(np.zeros(36))) == capi.CD_ERR_INVALID_ARG


# ---- the covariance of the published pose --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["view_three", "view_two", "six_faces"])
def test_ros_covariance_against_central_differences(name):
    """cd_pose_info_ros_covariance = J S J^T with J the derivative of (position, rotation about the parent's fixed axes) of
    P = (delta T)^-1 by the rule's (omega, t), here by central differences in float64 (step 1e-6: truncation 1e-12, rounding
    1e-10 relative).  T is a rotation to float32 precision only, which the helper's R_P = R_T^T inherits: 1e-6 relative."""
    case = [c for c in CASES if c[0] == name][0]
    o, T = spec(case), case[2]
    J = PR.numeric_ros_jacobian(T, o["centre"])
    S_ = np.array(o["covariance"]).reshape(6, 6)
    want = J @ S_ @ J.T
    got = capi.pose_info_ros_covariance(o, T)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    assert np.allclose(got, PI.ros_covariance(o, T), rtol=1e-12, atol=1e-30) and np.allclose(got, got.T, rtol=1e-12, atol=1e-30)
    assert np.linalg.eigvalsh(got).min() > -1e-12 * np.abs(got).max()
