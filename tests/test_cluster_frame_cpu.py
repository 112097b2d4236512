"""Rule C13 on the CPU (no GPU): the host entries cd_shape_frame_host / cd_shape_guess against the plain-Python restatement
perception_amd/cluster_frame.py, bit for bit in every field; the restatement's Jacobi against numpy.linalg.eigh; the ctypes
mirror of the new ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from perception_amd import capi, cluster_frame as cf, pcd, synth, templates

F32 = np.float32


def c_record(rec):
    """A restated record as the CdShapeFrame the C-ABI takes."""
    return capi.CdShapeFrame.from_buffer_copy(rec.to_bytes())


def same_record(points):
    a = np.asarray(points, F32)
    got, want = capi.shape_frame_host(a), cf.shape_frame(a)
    assert bytes(got) == want.to_bytes(), "n=%d status %d / %d" % (a.shape[0], got.status, want.status)
    return want


def four_templates():
    out = [templates.template_xyz32(**templates.DEFAULT_TEMPLATE)]
    for fn in ("template_cuboid_L200_W100_H75_3faces.pcd", "template_cuboid_L200_W75_H100_3faces.pcd", "template_cuboid_L200_W100_H75.pcd"):
        out.append(pcd.read_xyz(os.path.join(GOLDEN, fn)).astype(F32))
    return out


@pytest.fixture(scope="module")
def oracle_clusters(O, template):
    prm = capi.default_params()
    out = []
    for i in range(6):
        o = O.process_frame(synth.frame(i), prm, template, want_clouds=True)
        for k in range(o["result"].n_clusters):
            out.append(o["objects"][o["labels"] == k])
    assert len(out) >= 6
    return out


def random_clouds():
    rng = np.random.default_rng(20240613)
    out = []
    for n in (3, 4, 17, 200, 1401, 5000):
        R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        p = rng.standard_normal((n, 3)) * rng.uniform(0.001, 0.3, 3)
        out.append((p @ R.T + rng.uniform(-1.0, 1.0, 3)).astype(F32))
    out.append(rng.uniform(-64.0, 64.0, (3000, 3)).astype(F32))   # the whole of rule C4's range, both signs
    out.append(np.full((64, 3), 64.0, F32) * F32([1, -1, 1]))     # on the range's boundary (accepted: |x| <= 64)
    return out


def test_host_entry_equals_restatement_on_clusters_and_templates(oracle_clusters):
    for cl in oracle_clusters:
        assert same_record(cl).status == 0
    for t in four_templates():
        r = same_record(t)
        assert r.status == 0 and r.var[0] >= r.var[1] >= r.var[2]
    for p in random_clouds():
        assert same_record(p).status == 0
    # a stride: x, y, z are read at 0 / 4 / 8 of every record, whatever follows them
    wide = np.zeros((oracle_clusters[0].shape[0], 8), F32)
    wide[:, :3] = oracle_clusters[0]
    wide[:, 3:] = np.nan
    assert bytes(capi.shape_frame_host(wide)) == cf.shape_frame(oracle_clusters[0]).to_bytes()


def test_host_entry_equals_restatement_on_degenerate_sets():
    rng = np.random.default_rng(5)
    assert same_record(np.zeros((0, 3), F32)).status == capi.CD_ERR_FEW_CORRESPONDENCES
    assert same_record(rng.standard_normal((2, 3)).astype(F32)).status == capi.CD_ERR_FEW_CORRESPONDENCES
    assert same_record(rng.standard_normal((3, 3)).astype(F32)).status == 0
    equal = same_record(np.tile(F32([0.25, -0.5, 0.75]), (100, 1)))
    assert equal.status == 0 and equal.lo == [0.0] * 3 and equal.hi == [0.0] * 3
    assert equal.axes == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]   # nothing to rotate: every off-diagonal entry is 0 or skipped
    t = np.linspace(-1.0, 1.0, 41)[:, None]
    line = same_record((t * np.array([[0.3, -0.2, 0.1]]) + np.array([[0.1, 0.2, 0.5]])).astype(F32))
    # (not exactly 0: every mean of step 1 carries up to 2^-33 of fixed-point rounding, a covariance entry 2^-33 (1 + 2 |m|) <= 2^-32
    # with |m| <= 0.5, and a symmetric 3x3 perturbation of that size moves an eigenvalue by at most 3 * 2^-32; float32 rounding of
    # the points themselves adds ~1e-15)
    assert line.status == 0 and abs(line.var[1]) <= 3 * 2.0 ** -32 + 1e-12 and abs(line.var[2]) <= 3 * 2.0 ** -32 + 1e-12
    gx, gy = np.meshgrid(np.arange(-8, 9) / 64.0, np.arange(-4, 5) / 64.0)          # exactly planar, exactly representable
    plane = same_record(np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.5)], axis=1).astype(F32))
    assert plane.status == 0 and plane.var[2] == 0.0 and plane.lo[2] == 0.0 and plane.hi[2] == 0.0
    assert not np.signbit(plane.lo[2]) and not np.signbit(plane.hi[2])       # a zero extent is +0
    gx, gy, gz = np.meshgrid(np.arange(-4, 5) / 32.0, np.arange(-4, 5) / 32.0, np.arange(-1, 2) / 32.0)   # two equal variances
    sq = same_record(np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(F32))
    assert sq.status == 0 and sq.var[0] == sq.var[1] > sq.var[2]
    assert sq.axes == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]       # ties keep their order


def test_host_entry_refuses_like_the_restatement():
    rng = np.random.default_rng(6)
    good = rng.uniform(-1, 1, (50, 3)).astype(F32)
    for bad_value in (np.nan, np.inf, -np.inf, 64.00001, -65.0):
        for at in (0, 25, 49):
            p = good.copy()
            p[at, at % 3] = bad_value
            r = same_record(p)
            assert r.status == capi.CD_ERR_INVALID_ARG and r.n == 50 and not np.any(r.doubles())
    two = good[:2].copy()
    two[1, 2] = np.nan
    assert same_record(two).status == capi.CD_ERR_INVALID_ARG            # a refusal comes before "too few"
    lib = capi.load_library()
    out = capi.CdShapeFrame()
    assert lib.cd_shape_frame_host(None, 12, 5, C.byref(out)) == capi.CD_ERR_INVALID_ARG
    assert lib.cd_shape_frame_host(good.ctypes.data_as(C.c_void_p), 8, 5, C.byref(out)) == capi.CD_ERR_INVALID_ARG
    assert lib.cd_shape_frame_host(good.ctypes.data_as(C.c_void_p), 12, 5, None) == capi.CD_ERR_INVALID_ARG


def same_guess(c, t):
    G, flip = capi.shape_guess(c_record(c), c_record(t))
    Gr, flip_r = cf.guess(c, t)
    assert flip == flip_r and G.tobytes() == Gr.tobytes()
    return G, flip


def made_record(mean, axes=None, lo=(-0.1, -0.05, -0.01), hi=(0.11, 0.06, 0.02), status=0):
    r = cf.ShapeFrame(100, status)
    r.mean = [float(v) for v in mean]
    r.axes = [float(v) for v in (np.eye(3) if axes is None else np.asarray(axes)).ravel()]
    r.var = [3.0, 2.0, 1.0]
    r.lo, r.hi = [float(v) for v in lo], [float(v) for v in hi]
    return r


def test_guess_equals_restatement(oracle_clusters):
    tpls = [cf.shape_frame(t) for t in four_templates()]
    for cl in oracle_clusters:
        c = cf.shape_frame(cl)
        for t in tpls:
            G, flip = same_guess(c, t)
            assert flip >= 0 and np.all(G[3] == [0, 0, 0, 1])
            R = G[:3, :3].astype(np.float64)
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-6) and np.linalg.det(R) > 0.999       # a proper rotation
    # constructed: sigma = (1, 1, 1) (lo + hi < 0 on every axis), cluster axes = identity, so w = -mean and the winner is the F
    # whose signs are w's: each of the four wins once
    t = made_record([0.0, 0.0, 0.0], lo=(-0.11, -0.06, -0.02), hi=(0.1, 0.05, 0.01))
    for want, mean in ((0, [-1.0, -2.0, -3.0]), (1, [-1.0, 2.0, 3.0]), (2, [1.0, -2.0, 3.0]), (3, [1.0, 2.0, -3.0])):
        assert same_guess(made_record(mean), t)[1] == want
    # exact ties go to the first: w = (1, 0, 0) scores F0 = F1 = 1; w = (0, 0, -1) scores F1 = F2 = 1 > F0 = -1
    assert same_guess(made_record([-1.0, 0.0, 0.0]), t)[1] == 0
    assert same_guess(made_record([0.0, 0.0, 1.0]), t)[1] == 1
    # sigma = 0: an exactly symmetric axis has no say (here all three: every score is 0, the first F wins) ...
    sym = made_record([0.0, 0.0, 0.0], lo=(-0.1, -0.05, -0.01), hi=(0.1, 0.05, 0.01))
    assert same_guess(made_record([1.0, 2.0, -3.0]), sym)[1] == 0
    # ... and the threshold |lo + hi| <= 2^-20 (hi - lo) is kept on both sides: hi - lo = 2, lo + hi = 2^-19 (= 0) and the next double up
    at = made_record([0.0, 0.0, 0.0], lo=(-1.0 + 2.0 ** -20, -1.0, -1.0), hi=(1.0 + 2.0 ** -20, 1.0, 1.0))
    above = made_record([0.0, 0.0, 0.0], lo=(-1.0 + 2.0 ** -20, -1.0, -1.0), hi=(1.0 + 2.0 ** -20 + 2.0 ** -52, 1.0, 1.0))
    assert same_guess(made_record([-1.0, 0.0, 0.0]), at)[1] == 0          # sigma_0 = 0: all scores 0
    assert same_guess(made_record([-1.0, 0.0, 0.0]), above)[1] == 2       # sigma_0 = -1, w_0 = 1: F_0 = -1 wins, first of F2 / F3
    # the six-face template, whatever its sigma
    six = tpls[3]
    for cl in oracle_clusters[:3]:
        same_guess(cf.shape_frame(cl), six)
    # a rotated frame on both sides
    q = np.linalg.qr(np.random.default_rng(3).standard_normal((3, 3)))[0]
    q *= np.sign(np.linalg.det(q))
    same_guess(made_record([0.01, -0.02, 0.6], axes=q), made_record([-0.011, -0.011, -0.0107], axes=q.T, lo=(-0.09, -0.04, -0.01), hi=(0.11, 0.06, 0.027)))


def test_guess_identity_fallback():
    t = cf.shape_frame(templates.template_xyz32(**templates.DEFAULT_TEMPLATE))
    ok = made_record([0.0, 0.1, 0.6])
    eye = np.eye(4, dtype=F32)
    for c, tt in ((made_record([0.0, 0.1, 0.6], status=capi.CD_ERR_FEW_CORRESPONDENCES), t),
                  (ok, made_record([0.0, 0.0, 0.0], status=capi.CD_ERR_INVALID_ARG)),
                  (cf.shape_frame(np.zeros((2, 3), F32)), t),
                  (made_record([1e300, 0.0, 0.0]), t),                       # g overflows float32
                  (made_record([float("nan"), 0.0, 0.0]), t),
                  (ok, made_record([0.0, float("inf"), 0.0]))):
        G, flip = same_guess(c, tt)
        assert flip == -1 and np.array_equal(G, eye)
    lib = capi.load_library()
    g = np.zeros(16, F32)
    assert lib.cd_shape_guess(None, C.byref(c_record(t)), g.ctypes.data_as(C.POINTER(C.c_float)), None) == capi.CD_ERR_INVALID_ARG


def test_restated_jacobi_against_eigh(oracle_clusters):
    """Eigenvalues and axes (up to sign) of the restatement against numpy.linalg.eigh of the SAME covariance matrix (the rule's:
    fixed-point sums, double means).  Tolerance, derived and not fitted: with A the restated axes, L = diag(var) and
    r = ||C A - A L||_F + ||A^T A - I||_F ||C||_2 the residual of the Jacobi result, every var_i lies within r of an eigenvalue of C
    (Weyl / Bauer-Fike for a symmetric matrix); eigh's own backward error is of the order 8 eps ||C||_2.  So |var_i - lambda_i| <=
    tol = r + 8 eps ||C||_2, and an axis whose eigenvalue is separated from the others by gap g_i makes an angle theta with eigh's
    vector where sin(theta) <= 2 tol / g_i (Davis-Kahan); a bound >= 1 says nothing and is not asserted."""
    eps = np.finfo(np.float64).eps
    sets = list(oracle_clusters) + four_templates() + random_clouds()
    worst = 0.0
    for p in sets:
        rec = cf.shape_frame(p)
        assert rec.status == 0
        S = cf.moments(p)
        n = float(rec.n)
        m = [(float(S[a]) * 2.0 ** -32) / n for a in range(3)]
        e = [(float(S[3 + k]) * 2.0 ** -32) / n for k in range(6)]
        Cm = np.zeros((3, 3))
        for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            Cm[a, b] = Cm[b, a] = e[k] - m[a] * m[b]
        A = np.array(rec.axes).reshape(3, 3)
        L = np.array(rec.var)
        norm = np.linalg.norm(Cm, 2)
        r = np.linalg.norm(Cm @ A - A * L) + np.linalg.norm(A.T @ A - np.eye(3)) * norm
        tol = r + 8 * eps * norm
        w, v = np.linalg.eigh(Cm)
        w, v = w[::-1], v[:, ::-1]
        assert np.all(np.abs(w - L) <= tol), (w, L, tol)
        assert r <= 64 * eps * norm                      # eight sweeps have converged: the residual is rounding error
        assert abs(np.linalg.det(A) - 1.0) <= 64 * eps   # right-handed
        for i in range(3):
            gap = min(abs(w[i] - w[j]) for j in range(3) if j != i)
            if gap > 0 and 2 * tol / gap < 1.0:
                sin = float(np.linalg.norm(A[:, i] - (A[:, i] @ v[:, i]) * v[:, i]))   # (not sqrt(1 - cos^2): that is only good to sqrt(eps))
                assert sin <= 2 * tol / gap + 8 * eps, (i, sin, tol, gap)
        worst = max(worst, r / max(norm, 1e-300))
    print("largest relative Jacobi residual %.3g" % worst)


def test_ctypes_mirror_of_the_new_abi():
    lib = capi.load_library()
    for name in ("cd_shape_frame_struct_size", "cd_shape_frame_host", "cd_shape_frames", "cd_template_shape_frame", "cd_shape_guess",
                 "cd_get_cluster_shape_frames"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert capi.CD_GUESS_CLUSTER == 4 and capi.CD_FRAME_CLUSTER_GUESS == 4
    assert lib.cd_shape_frame_struct_size() == C.sizeof(capi.CdShapeFrame) == 176
    hdr = open(os.path.join(ROOT, "include", "cuboid_hip.h")).read()
    assert re.search(r"CD_GUESS_CLUSTER\s*=\s*4\b", hdr) and re.search(r"#define\s+CD_FRAME_CLUSTER_GUESS\s+4\b", hdr)
    assert lib.cd_abi_version() == 4                                    # nothing existing changed
    assert lib.cd_struct_size(0) == C.sizeof(capi.CdParams) and lib.cd_struct_size(2) == C.sizeof(capi.CdFrameResult)
    assert (cf.CD_OK, cf.CD_ERR_INVALID_ARG, cf.CD_ERR_CAPACITY, cf.CD_ERR_FEW_CORRESPONDENCES) == \
           (capi.CD_OK, capi.CD_ERR_INVALID_ARG, capi.CD_ERR_CAPACITY, capi.CD_ERR_FEW_CORRESPONDENCES)
