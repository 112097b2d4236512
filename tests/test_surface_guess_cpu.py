"""CPU checks of rule C9: cd_surface_guess against a plain restatement, bit for bit, on surface poses the
oracle's surface_frame computes and on perturbed, nearly orthonormal matrices; its refusal of non-finite input; and the
ctypes mirror of the CD_GUESS_SURFACE additions."""
import ctypes as C
import math

import numpy as np
import pytest

from perception_amd import capi, synth

FLIPS = ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))


def pose_quaternion(H):
    """cd_pose_to_position_quaternion (tf::Matrix3x3::getRotation) in Python doubles."""
    m = [[H[0], H[1], H[2]], [H[4], H[5], H[6]], [H[8], H[9], H[10]]]
    trace = m[0][0] + m[1][1] + m[2][2]
    t = [0.0] * 4
    if trace > 0.0:
        s = math.sqrt(trace + 1.0)
        t[3] = s * 0.5
        s = 0.5 / s
        t[0] = (m[2][1] - m[1][2]) * s
        t[1] = (m[0][2] - m[2][0]) * s
        t[2] = (m[1][0] - m[0][1]) * s
    else:
        i = (2 if m[1][1] < m[2][2] else 1) if m[0][0] < m[1][1] else (2 if m[0][0] < m[2][2] else 0)
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        t[i] = s * 0.5
        s = 0.5 / s
        t[3] = (m[k][j] - m[j][k]) * s
        t[j] = (m[j][i] + m[i][j]) * s
        t[k] = (m[k][i] + m[i][k]) * s
    return [H[3], H[7], H[11]], t


def c9(Rt):
    """Rule C9, step by step; returns (guess float32 4x4, index of the chosen F) or None for a refused input."""
    Rt = np.asarray(Rt, np.float32).reshape(16)
    if not np.all(np.isfinite(Rt)):
        return None
    H = [float(v) for v in Rt]
    t, (x, y, z, w) = pose_quaternion(H)
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    best, best_score = 0, -1
    for k, Fk in enumerate(FLIPS):
        score = sum(1 for a in range(3) if (R[0][a] * Fk[a] * t[0] + R[1][a] * Fk[a] * t[1]) + R[2][a] * Fk[a] * t[2] > 0.0)
        if score > best_score:
            best, best_score = k, score
    M = [[R[r][a] * FLIPS[best][a] for a in range(3)] for r in range(3)]
    G = np.zeros((4, 4), np.float32)
    for i in range(3):
        for j in range(3):
            G[i, j] = np.float32(M[j][i])
        G[i, 3] = np.float32(-((M[0][i] * t[0] + M[1][i] * t[1]) + M[2][i] * t[2]))
    G[3, 3] = 1.0
    if not np.all(np.isfinite(G)):
        return None
    return G, best


def scene_with_yaw(i, yaw_deg):
    """synth.scene_for(i, k_obj=1) with the box's yaw overridden, R rebuilt as scene_for builds it."""
    sc = synth.scene_for(i, k_obj=1)
    bx = sc["boxes"][0]
    yaw = np.deg2rad(yaw_deg)
    ex = np.cos(yaw) * sc["e1"] + np.sin(yaw) * sc["e2"]
    ey = np.cross(sc["n"], ex)
    bx["R"] = np.stack([ex, ey, sc["n"]], axis=1)
    bx["yaw"] = yaw
    return sc


PRECHECK = ((0, 0.0), (1, 30.0), (2, 60.0), (3, 85.0), (4, -70.0), (5, 45.0))


def _check(Rt):
    ref = c9(Rt)
    assert ref is not None
    got = capi.surface_guess(Rt)
    assert np.array_equal(got.view(np.uint32), ref[0].view(np.uint32)), (Rt, got, ref[0])
    return ref[1]


def test_surface_guess_matches_restatement_on_oracle_poses(O, template):
    """The surface poses the oracle's sne derives from the pre-check frames' objects clouds."""
    prm = capi.default_params()
    sne = capi.default_params()
    sne.plane_distance_threshold = 0.004
    n_ok = 0
    for i, yaw in PRECHECK:
        o = O.process_frame(synth.render(scene_with_yaw(i, yaw)), prm, template, want_clouds=True)
        r = o["result"]
        if r.n_objects < 3:
            continue
        st, res = O.surface_frame(o["objects"], np.array(r.plane[:3], np.float32), sne, invert=True)
        if st != capi.CD_OK:
            continue
        n_ok += 1
        _check(np.array(res.Rt, np.float32))
    assert n_ok >= 3


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_surface_guess_matches_restatement_perturbed():
    """Nearly orthonormal matrices (sne fits its three normals independently) and positions around the camera."""
    rng = np.random.default_rng(9)
    for _ in range(400):
        Rt = np.eye(4)
        Rt[:3, :3] = _rot(rng) + rng.normal(scale=0.02, size=(3, 3))
        Rt[:3, 3] = rng.normal(scale=0.3, size=3) + np.array([0.0, 0.0, 0.5])
        _check(Rt.astype(np.float32))


def test_surface_guess_exercises_every_flip_and_the_tie():
    """Step 3: positions chosen so that each F wins, and a tie (score equal for several F: the first is taken)."""
    seen = set()
    for k, Fk in enumerate(FLIPS):
        # R = I: column a of R F is Fk[a] e_a, so t = 0.3 Fk scores 3 for Fk and 1 for every other F
        Rt = np.eye(4, dtype=np.float32)
        Rt[:3, 3] = np.array(Fk, np.float32) * np.float32(0.3)
        assert _check(Rt) == k
        seen.add(k)
    assert seen == {0, 1, 2, 3}
    Rt = np.eye(4, dtype=np.float32)   # t = 0: every score is 0, the tie goes to F = I
    assert _check(Rt) == 0
    Rt[:3, 3] = (0.0, 0.0, -0.5)      # only z decides: I and diag(-1,-1,1) score 0, diag(1,-1,-1) and diag(-1,1,-1) 1
    assert _check(Rt) == 1


def test_surface_guess_rejects_non_finite():
    lib = capi.load_library()
    f32 = C.POINTER(C.c_float)
    g = np.full(16, 7.0, np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        Rt = np.eye(4, dtype=np.float32).reshape(16)
        Rt[5] = bad
        assert lib.cd_surface_guess(Rt.ctypes.data_as(f32), g.ctypes.data_as(f32)) == capi.CD_ERR_INVALID_ARG
        assert np.all(g == 7.0)   # untouched
        with pytest.raises(capi.CuboidError):
            capi.surface_guess(Rt)


def test_ctypes_mirror_of_the_surface_additions():
    assert capi.CD_GUESS_SURFACE == 3
    assert capi.CD_FRAME_SURFACE_GUESS == 2
    assert capi.CD_FRAME_SURFACE_GUESS & capi.CD_FRAME_MORE_CLUSTERS == 0
    for name in ("cd_surface_batch", "cd_surface_guess", "cd_set_surface_distance_threshold",
                 "cd_get_surface_distance_threshold", "cd_get_surface_results"):
        assert name in capi.EXPORTED_SYMBOLS
    lib = capi.load_library()
    assert len(lib.cd_surface_batch.argtypes) == 11
    assert lib.cd_surface_batch.argtypes[9] is C.POINTER(capi.CdSurfaceFrameResult)
    assert len(lib.cd_get_surface_results.argtypes) == 5
    assert lib.cd_set_surface_distance_threshold.argtypes[1] is C.c_double
    assert lib.cd_abi_version() == capi.CD_ABI_VERSION == 4
