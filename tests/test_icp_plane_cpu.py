"""Rule C17 (plane-weighted ICP for lattice templates) without a GPU: the numpy module (perception_amd/icp_plane.py) against an
exact restatement with Python integers and fractions and a hand-derived iteration, the host arithmetic of icp_plane_math.hpp
(icp_plane_math_check, plain and sanitized, and cd_icp_plane_solve_host) against the module bit for bit, the module's behaviour
against the oracle's point-to-point ICP on synth clusters, and the names the header and capi.py export."""
import os
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN
from perception_amd import capi, cluster_frame as cf, icp_plane as IP, pcd, synth, templates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "perception_amd", "csrc")
NEW_SYMBOLS = ["cd_set_icp_plane_weight", "cd_get_icp_plane_weight", "cd_get_cluster_plane_stats", "cd_icp_plane_solve_host"]
PRM = dict(icp_max_iterations=5000, icp_transformation_epsilon=1e-9, icp_euclidean_fitness_epsilon=0.0004, icp_accept_fitness=0.0004)
EYE = np.eye(4, dtype=np.float32)


def test_header_and_capi_export_the_names():
    header = open(os.path.join(ROOT, "include", "cuboid_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS, name
    assert re.search(r"#define CD_ICP_PLANE_WEIGHT_DEFAULT \(1\.0 / 32\.0\)", header)
    assert re.search(r"#define CD_ICP_PLANE_SWITCH_DEFAULT 0\.01\b", header)
    assert re.search(r"typedef struct cd_icp_plane_stats", header) and "TransformationEstimationPointToPlaneLLS" in header
    assert capi.CD_ICP_PLANE_WEIGHT_DEFAULT == IP.TANGENT_WEIGHT_DEFAULT == 1.0 / 32.0
    assert capi.CD_ICP_PLANE_SWITCH_DEFAULT == IP.SWITCH_DISTANCE_DEFAULT == 0.01
    assert capi.CD_ICP_PLANE_WEIGHT_MIN == IP.TANGENT_WEIGHT_MIN == 1.0 / 1024.0
    assert re.search(r"#define CD_ABI_VERSION 4\b", header)
    p = capi.default_params()
    assert {k: getattr(p, k) for k in PRM} == PRM   # the behaviour tests below run the default parameters
    for fn in (capi.Context.set_icp_plane_weight, capi.Context.icp_plane_weight, capi.Context.cluster_plane_stats, capi.icp_plane_solve_host):
        assert callable(fn)


@pytest.fixture(scope="module")
def tpl():
    return templates.template_xyz32(**templates.DEFAULT_TEMPLATE)


@pytest.fixture(scope="module")
def axes(tpl):
    return IP.face_axes(tpl)


def test_face_axes_equal_the_library_lattice_detection(tpl):
    for t in [tpl] + [pcd.read_xyz(os.path.join(GOLDEN, f)) for f in ("template_cuboid_L200_W100_H75.pcd", "template_cuboid_L200_W100_H75_3faces.pcd",
                                                                      "template_cuboid_L200_W75_H100_3faces.pcd")]:
        ref = np.full(len(t), -1, np.int32)
        for (w, _u, base, nfast, nslow) in capi.lattice_detect(t):
            ref[base:base + nfast * nslow] = w
        assert np.array_equal(IP.face_axes(t), ref)
    with pytest.raises(ValueError):
        IP.face_axes(pcd.read_xyz(os.path.join(GOLDEN, "eraser_ascii.pcd")))


# ---- sums to solve: the cases every comparison below shares -------------------------------------------------------------------------
def correspondences(tpl, axes, n, seed, noise=0.002, scale=1.0, offset=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    sel = rng.choice(len(tpl), n, replace=False)
    S = ((tpl[sel] + rng.normal(0, noise, (n, 3))) * scale + np.asarray(offset)).astype(np.float32)
    idx, d2 = IP.nearest(tpl, S)
    return S, tpl[idx], axes[idx], d2


def well_posed_sums(tpl, axes, count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(12, 200))
        S, Q, W, d2 = correspondences(tpl, axes, n, seed * 100003 + i, noise=float(rng.uniform(0.0002, 0.004)))
        lam = np.float32(rng.choice([1.0, 1.0 / 32.0, 1.0 / 1024.0, 0.3]))
        out.append((IP.sums(IP.terms(S, Q, W, d2, lam)), n))
    return out


def dyadic_line(n=81):
    """Points on one line parallel to the bottom face, 0.6 mm below it, with coordinates on a 2^-9 grid: every term of M is exact
    in float32 and in the sums, so the system is EXACTLY singular (the rotation about the line is free).  A line with arbitrary
    coordinates is singular only up to the float32 rounding of its terms (1e-7 of the diagonal), far above the rule's 2^-40."""
    x = (np.arange(n, dtype=np.float32) - np.float32(n // 2)) * np.float32(2.0 ** -9)
    return np.stack([x, np.full(n, 2.0 ** -6, np.float32), np.full(n, -2.0 ** -6, np.float32)], 1).astype(np.float32)


def degenerate_sums(tpl, axes):
    out = [(np.zeros(28, np.int64), 0), (np.zeros(28, np.int64), 5)]
    S, Q, W, d2 = correspondences(tpl, axes, 1, 1)
    out.append((IP.sums(IP.terms(np.repeat(S, 9, 0), np.repeat(Q, 9, 0), np.repeat(W, 9), np.repeat(d2, 9), 1.0 / 32.0)), 9))   # one point repeated
    line = tpl[:40]   # collinear: one row of the bottom face
    out.append((IP.sums(IP.terms(line + np.float32([0, 0, 0.001]), line, axes[:40], np.full(40, 1e-6, np.float32), 1.0 / 32.0)), 40))
    out.append((IP.sums(IP.terms(line, line, axes[:40], np.zeros(40, np.float32), 1.0)), 40))
    S, Q, W, d2 = correspondences(tpl, axes, 60, 2, scale=1.0, offset=(900.0, -700.0, 800.0))   # huge coordinates: the general conversion
    out.append((IP.sums(IP.terms(S, Q, W, d2, 1.0 / 32.0)), 60))
    S, Q, W, d2 = correspondences(tpl, axes, 50, 3, scale=300.0)
    out.append((IP.sums(IP.terms(S, Q, W, d2, 1.0)), 50))
    for lam in (1.0, 1.0 / 32.0):   # an exactly singular line
        S = dyadic_line()
        idx, d2 = IP.nearest(tpl, S)
        out.append((IP.sums(IP.terms(S, tpl[idx], axes[idx], d2, lam)), len(S)))
    bottom = np.nonzero(axes == 2)[0][::37]   # one face, tangential weight 0 emulated by the sums: singular
    out.append((IP.sums(IP.terms(tpl[bottom] + np.float32([0, 0, 0.001]), tpl[bottom], axes[bottom], np.full(len(bottom), 1e-6, np.float32), 0.0)), len(bottom)))
    return out


def exact_solve(A):
    """Steps 3 and 4 in exact rational arithmetic from the integer sums: nothing shared with the module but the rule's text."""
    s = [Fraction(int(v), 2 ** 32) for v in A[:27]]
    M = [[Fraction(0)] * 6 for _ in range(6)]
    b = [Fraction(0)] * 6
    for a in range(3):
        ob, oc, ta = (a + 1) % 3, (a + 2) % 3, 3 + a
        S = s[9 * a:9 * a + 9]
        M[ob][ob] += S[3]
        M[oc][oc] += S[4]
        M[ob][oc] -= S[5]
        M[oc][ob] -= S[5]
        M[ob][ta] += S[1]
        M[ta][ob] += S[1]
        M[oc][ta] -= S[2]
        M[ta][oc] -= S[2]
        M[ta][ta] += S[0]
        b[ob] += S[7]
        b[oc] -= S[8]
        b[ta] += S[6]
    aug = [row[:] + [bi] for row, bi in zip(M, b)]
    for j in range(6):   # Gauss-Jordan, no pivoting: M is positive definite for the cases this is called with
        piv = aug[j][j]
        assert piv != 0
        aug[j] = [v / piv for v in aug[j]]
        for i in range(6):
            if i != j and aug[i][j] != 0:
                f = aug[i][j]
                aug[i] = [vi - f * vj for vi, vj in zip(aug[i], aug[j])]
    x = [aug[i][6] for i in range(6)]
    kx, ky, kz = x[0] / 2, x[1] / 2, x[2] / 2
    m = 1 + kx * kx + ky * ky + kz * kz
    R = [[(1 + kx * kx - ky * ky - kz * kz) / m, 2 * (kx * ky - kz) / m, 2 * (kx * kz + ky) / m],
         [2 * (kx * ky + kz) / m, (1 - kx * kx + ky * ky - kz * kz) / m, 2 * (ky * kz - kx) / m],
         [2 * (kx * kz - ky) / m, 2 * (ky * kz + kx) / m, (1 - kx * kx - ky * ky + kz * kz) / m]]
    T = np.zeros((4, 4), np.float64)
    for i in range(3):
        for j in range(3):
            T[i, j] = float(R[i][j])
        T[i, 3] = float(x[3 + i])
    T[3, 3] = 1.0
    return T


def test_solve_equals_the_exact_restatement_and_is_a_rotation(tpl, axes):
    for A, n in well_posed_sums(tpl, axes, 40, 5):
        T, singular = IP.solve(A, n)
        assert singular == 0
        E = exact_solve(A)
        # the double solve is good to 1e-9 relative on these systems; the cast to float32 adds half an ulp
        tol = np.abs(E) * (2.0 ** -24 + 1e-9) + 1e-12
        assert np.all(np.abs(T.astype(np.float64) - E) <= tol), (T, E)
        R = T[:3, :3].astype(np.float64)
        assert np.abs(R.T @ R - np.eye(3)).max() <= 4 * 2.0 ** -23 and abs(np.linalg.det(R) - 1.0) <= 4 * 2.0 ** -23
        assert list(T[3]) == [0, 0, 0, 1]


def test_one_face_without_tangential_weight_is_singular(tpl, axes):
    A, n = degenerate_sums(tpl, axes)[-1]
    T, singular = IP.solve(A, n)
    assert singular == 1 and np.array_equal(T, EYE)
    # the same correspondences with the rule's least weight are not
    bottom = np.nonzero(axes == 2)[0][::37]
    A = IP.sums(IP.terms(tpl[bottom] + np.float32([0, 0, 0.001]), tpl[bottom], axes[bottom], np.full(len(bottom), 1e-6, np.float32), 1.0 / 1024.0))
    assert IP.solve(A, len(bottom))[1] == 0
    # nothing to solve, and a line (rotation about it is free)
    assert IP.solve(np.zeros(28, np.int64), 0)[1] == 1 and IP.solve(np.zeros(28, np.int64), 7)[1] == 1
    for A, n in degenerate_sums(tpl, axes)[-3:-1]:
        assert IP.solve(A, n)[1] == 1
    S = dyadic_line()
    assert np.all(axes[IP.nearest(tpl, S)[0]] == 2)
    for sw in (np.inf, 0.01):
        r = IP.icp(tpl, axes, S, PRM, 1.0 / 32.0, sw)
        assert (r.stopped_singular, r.iterations, r.converged, r.accepted) == (1, 0, 0, 0)
        assert np.array_equal(r.T, EYE) and np.array_equal(r.aligned, S) and (r.plane_iterations, r.first_plane_iteration) == (0, 0)


# ---- the host arithmetic of icp_plane_math.hpp -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["", "-fsanitize=address,undefined"], ids=["plain", "sanitized"])
def check_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("icp_plane") / "icp_plane_math_check")
    cmd = ["g++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
           "-Wno-unknown-pragmas"] + ([request.param] if request.param else []) + [os.path.join(CSRC, "icp_plane_math_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def _run(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().split("\n")


@pytest.fixture(scope="module")
def solve_cases(tpl, axes):
    cases = well_posed_sums(tpl, axes, 2500, 7) + degenerate_sums(tpl, axes)
    return cases, [IP.solve(A, n) for A, n in cases]


def test_check_program_solve_equals_the_module_bitwise(check_exe, tmp_path, solve_cases):
    cases, expected = solve_cases
    path = str(tmp_path / "solve.bin")
    with open(path, "wb") as fp:
        fp.write(struct.pack("<ii", 0, len(cases)))
        for A, n in cases:
            fp.write(np.asarray(A, "<i8").tobytes() + struct.pack("<ii", n, 0))
    lines = _run(check_exe, path)
    assert len(lines) == len(cases)
    n_singular = 0
    for line, (T, singular) in zip(lines, expected):
        w = line.split()
        assert w[0] == "T" and int(w[17]) == singular
        assert [int(v, 16) for v in w[1:17]] == T.view(np.uint32).ravel().tolist()
        n_singular += singular
    assert 5 <= n_singular < 12


def test_library_host_solve_equals_the_module_bitwise(solve_cases):
    cases, expected = solve_cases
    for (A, n), (T, singular) in list(zip(cases, expected))[::25] + list(zip(cases, expected))[-8:]:
        Tl, sl = capi.icp_plane_solve_host(A, n)
        assert sl == singular and Tl.view(np.uint32).tolist() == T.view(np.uint32).tolist()


def test_check_program_terms_equal_the_module_bitwise(check_exe, tmp_path, tpl, axes):
    parts = [correspondences(tpl, axes, 3000, 11), correspondences(tpl, axes, 500, 12, noise=0.05),
             correspondences(tpl, axes, 300, 13, offset=(900.0, -700.0, 800.0)), correspondences(tpl, axes, 300, 14, scale=300.0),
             (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), np.array([0, 1, 2, 0]), np.zeros(4, np.float32))]
    S, Q, W, d2 = (np.concatenate([p[i] for p in parts], 0) for i in range(4))
    rng = np.random.default_rng(15)
    lam = rng.choice(np.float32([1.0, 1.0 / 32.0, 1.0 / 1024.0, 0.3]), len(S)).astype(np.float32)
    expected = np.empty((len(S), 28), np.float32)
    for v in np.unique(lam):
        m = lam == v
        expected[m] = IP.terms(S[m], Q[m], W[m], d2[m], v)
    path = str(tmp_path / "terms.bin")
    with open(path, "wb") as fp:
        fp.write(struct.pack("<ii", 1, len(S)))
        rec = np.zeros(len(S), np.dtype([("s", "<f4", 3), ("q", "<f4", 3), ("lam", "<f4"), ("d2", "<f4"), ("w", "<i4"), ("pad", "<i4")]))
        rec["s"], rec["q"], rec["lam"], rec["d2"], rec["w"] = S, Q, lam, d2, W
        fp.write(rec.tobytes())
    lines = _run(check_exe, path)
    assert len(lines) == len(S) + 1
    got = np.array([[int(v, 16) for v in line.split()[1:]] for line in lines[:-1]], np.uint32)
    assert np.array_equal(got, expected.view(np.uint32))
    sums = np.array([int(v, 16) for v in lines[-1].split()[1:]], np.uint64)
    assert lines[-1].startswith("sums") and np.array_equal(sums, IP.sums(expected).view(np.uint64))
    assert np.abs(expected[:, :27]).max() > 2.0 ** 18   # some terms lie outside the raw-bits conversion's range


def test_check_program_refuses_a_file_it_cannot_read(check_exe, tmp_path):
    path = str(tmp_path / "short.bin")
    with open(path, "wb") as fp:
        fp.write(struct.pack("<ii", 0, 3) + b"\0" * 100)
    assert subprocess.run([check_exe, path], capture_output=True).returncode == 2


# ---- one iteration by hand -------------------------------------------------------------------------------------------------------------
def test_a_translated_face_subset_moves_back_by_the_offset(tpl, axes):
    """Interior points of the bottom face (constant z) lifted by delta: every correspondence is the point's own lattice point,
    every residual is (0, 0, -delta'), so the least-squares step is the translation (0, 0, -delta') and no rotation, whatever
    the tangential weight."""
    bottom = np.nonzero(axes == 2)[0].reshape(50, 100)[10:40:3, 10:90:3].ravel()
    delta = np.float32(0.0005)
    src = (tpl[bottom] + np.float32([0, 0, delta])).astype(np.float32)
    d_eff = float(np.float32(src[0, 2] - tpl[bottom[0], 2]))   # delta as float32 subtraction sees it
    prm = dict(PRM, icp_max_iterations=1)
    for sw in (np.inf, 0.0):
        r = IP.icp(tpl, axes, src, prm, 1.0 / 32.0, sw)
        assert (r.iterations, r.converged, r.stopped_singular) == (1, 1, 0)
        assert r.first_plane_iteration == (1 if np.isinf(sw) else 0)
        T = r.T.astype(np.float64)
        assert abs(T[2, 3] + d_eff) <= 1e-9 and abs(T[0, 3]) <= 1e-9 and abs(T[1, 3]) <= 1e-9
        assert np.abs(T[:3, :3] - np.eye(3)).max() <= 1e-7
        assert np.abs(r.aligned - tpl[bottom]).max() <= 2e-7


# ---- behaviour, mirror only ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth_runs(tpl, axes):
    """The oracle's clusters of synth.frame(0..3): the oracle's point-to-point ICP and the module's plane-weighted one at the
    recommended setting, both from the rule-C13 cluster guess."""
    from oracle import oracle_py as O
    t_rec = cf.shape_frame(tpl)
    prm = capi.default_params()
    runs = []
    for i in range(4):
        o = O.process_frame(synth.frame(i), prm, tpl, want_clouds=True)
        for k in range(o["result"].n_clusters):
            src = o["objects"][o["labels"] == k]
            G, _ = cf.guess(cf.shape_frame(src), t_rec)
            p = capi.default_params()
            p.icp_use_guess = capi.CD_GUESS_PARAMS
            p.icp_guess[:] = [float(v) for v in G.ravel()]
            _, r, _ = O.icp(tpl, src, p)
            m = IP.icp(tpl, axes, src, prm, IP.TANGENT_WEIGHT_DEFAULT, IP.SWITCH_DISTANCE_DEFAULT, guess=np.asarray(G, np.float32))
            runs.append((src, r, m))
    return runs


def test_mirror_accepts_what_the_oracle_accepts_in_fewer_iterations(synth_runs):
    assert len(synth_runs) >= 4
    oracle_total = sum(r.iterations for _, r, _ in synth_runs)
    plane_total = sum(m.iterations for _, _, m in synth_runs)
    print("ICP iterations from the cluster guess, %d clusters: point-to-point (oracle) %d, plane-weighted (1/32, 0.01) %d"
          % (len(synth_runs), oracle_total, plane_total))
    for _, r, m in synth_runs:
        assert m.accepted or not r.accepted
        assert m.stopped_singular == 0
    assert plane_total < oracle_total


def test_latch(synth_runs, tpl, axes):
    prm = capi.default_params()
    src = synth_runs[0][0]   # as extracted: about 0.55 m from the object-centred template
    far = IP.icp(tpl, axes, src, prm, 1.0 / 32.0, 0.01)
    assert far.first_plane_iteration > 1 and far.converged == 1
    at_once = IP.icp(tpl, axes, src, dict(PRM, icp_max_iterations=6), 1.0 / 32.0, np.inf)
    assert at_once.first_plane_iteration == 1 and at_once.plane_iterations == at_once.iterations
    never = IP.icp(tpl, axes, src, dict(PRM, icp_max_iterations=3), 1.0 / 32.0, 0.0)
    assert (never.first_plane_iteration, never.plane_iterations) == (0, 0)
    latched = [m for _, _, m in synth_runs] + [far]
    assert all(m.first_plane_iteration > 0 for m in latched)
    for m in latched:   # the latch never reopens
        assert m.plane_iterations == m.iterations - m.first_plane_iteration + 1
