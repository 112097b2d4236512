"""Rule C11 without a GPU: the numpy restatement (perception_amd/overlay.py) against pixel sets written out by hand, the
host-only cd_overlay_project against the restatement bit for bit, and the ctypes mirror of the two new structs."""
import ctypes as C

import numpy as np
import pytest

from perception_amd import capi, overlay, synth

EYE_P = (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0)   # u = x / z, v = y / z


def _set(mask):
    ys, xs = np.nonzero(mask)
    return {(int(x), int(y)) for x, y in zip(xs, ys)}


# ---- step 6: pixel sets by hand ------------------------------------------------------------------------------------------
def test_thickness_1_horizontal():
    assert _set(overlay.segment_mask(8, 6, (2, 3), (5, 3), 1)) == {(2, 3), (3, 3), (4, 3), (5, 3)}
    assert _set(overlay.segment_mask(8, 6, (5, 3), (2, 3), 1)) == {(2, 3), (3, 3), (4, 3), (5, 3)}


def test_thickness_1_vertical():
    assert _set(overlay.segment_mask(8, 6, (4, 1), (4, 4), 1)) == {(4, 1), (4, 2), (4, 3), (4, 4)}


def test_thickness_1_diagonal():
    assert _set(overlay.segment_mask(8, 6, (1, 1), (4, 4), 1)) == {(1, 1), (2, 2), (3, 3), (4, 4)}
    assert _set(overlay.segment_mask(8, 6, (4, 1), (1, 4), 1)) == {(4, 1), (3, 2), (2, 3), (1, 4)}


def test_thickness_1_degenerate():
    assert _set(overlay.segment_mask(8, 6, (3, 2), (3, 2), 1)) == {(3, 2)}


def test_thickness_2_horizontal_three_rows_and_round_caps():
    want = {(x, y) for x in range(2, 6) for y in (2, 3, 4)} | {(1, 3), (6, 3)}
    assert _set(overlay.segment_mask(8, 6, (2, 3), (5, 3), 2)) == want


def test_thickness_2_degenerate_is_a_plus():
    assert _set(overlay.segment_mask(8, 6, (3, 2), (3, 2), 2)) == {(3, 2), (2, 2), (4, 2), (3, 1), (3, 3)}


def test_segment_crossing_the_border_paints_only_inside():
    assert _set(overlay.segment_mask(6, 5, (-3, 2), (2, 2), 1)) == {(0, 2), (1, 2), (2, 2)}
    want = {(4, 0), (4, 1), (3, 0), (5, 0), (3, 1), (5, 1), (4, 2)}
    assert _set(overlay.segment_mask(6, 5, (4, -1), (4, 1), 2)) == want
    assert _set(overlay.segment_mask(6, 5, (-9, -9), (-2, -2), 3)) == set()
    assert _set(overlay.segment_mask(1, 1, (-5, 0), (5, 0), 1)) == {(0, 0)}


# ---- steps 3 and 4 --------------------------------------------------------------------------------------------------------
def test_truncation_toward_zero():
    M = overlay.matrix(EYE_P, overlay.DEFAULT_E)
    assert overlay.project_point(M, (-0.5, -0.9, 1.0)) == (0, 0)
    assert overlay.project_point(M, (1.9, -1.5, 1.0)) == (1, -1)
    assert overlay.project_point(M, (-3.0, 5.0, 2.0)) == (-1, 2)


def _point_pose(x, y, z):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


def test_the_three_skip_conditions():
    zero = (0.0, 0.0, 0.0)   # every corner is the pose's translation
    assert overlay.project(_point_pose(3.0, 4.0, 1.0), EYE_P, dims=zero) == ([3, 4] * 8, 1)
    # a non-finite u or v
    bad = np.eye(4)
    bad[0, 0] = np.nan
    assert overlay.project(bad, dims=overlay.DEFAULT_DIMS) == ([0] * 16, 0)
    assert overlay.project(_point_pose(np.inf, 0.0, 1.0), EYE_P, dims=zero) == ([0] * 16, 0)
    # h_2 <= 0
    assert overlay.project(_point_pose(0.1, 0.1, -1.0), EYE_P, dims=zero) == ([0] * 16, 0)
    assert overlay.project(_point_pose(0.1, 0.1, 0.0), EYE_P, dims=zero) == ([0] * 16, 0)
    # |pixel coordinate| > 8192
    assert overlay.project(_point_pose(8192.5, -8192.5, 1.0), EYE_P, dims=zero) == ([8192, -8192] * 8, 1)
    assert overlay.project(_point_pose(8193.0, 0.0, 1.0), EYE_P, dims=zero) == ([0] * 16, 0)
    assert overlay.project(_point_pose(0.0, -8193.0, 1.0), EYE_P, dims=zero) == ([0] * 16, 0)
    # one corner behind the camera skips the whole box
    assert overlay.project(_point_pose(0.0, 0.0, 0.01), dims=(0.2, 0.1, 0.03))[1] == 0


def test_edges_and_corner_order():
    assert overlay.EDGES == ((0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7))
    c = overlay.corners(np.eye(4), (2.0, 4.0, 6.0))
    want = [(-1, -2, -3), (-1, -2, 3), (-1, 2, -3), (-1, 2, 3), (1, -2, -3), (1, -2, 3), (1, 2, -3), (1, 2, 3)]
    assert c.dtype == np.float32 and [tuple(r) for r in c] == want


def test_draw_touches_only_painted_pixels_and_one_colour():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (2, 48, 64, 3)).astype(np.uint8)
    P = (60.0, 0, 32.0, 0, 0, 60.0, 24.0, 0, 0, 0, 1.0, 0)
    poses = np.stack([_point_pose(0.0, 0.0, 1.0), _point_pose(0.3, 0.1, 1.2)])[None].repeat(2, 0)
    out, boxes, painted = overlay.draw(img, poses, n_boxes=[2, 1], P=P, dims=(0.4, 0.3, 0.2), thickness=3, rgb=(9, 8, 7))
    assert boxes[0, :, 16].tolist() == [1, 1] and boxes[1, :, 16].tolist() == [1, 0] and not boxes[1, 1].any()
    assert painted[0].sum() > painted[1].sum() > 0
    assert (out[painted] == (9, 8, 7)).all() and np.array_equal(out[~painted], img[~painted])
    assert np.array_equal(painted[1], overlay.box_mask(64, 48, boxes[1, 0, :16], 3))


# ---- cd_overlay_project == overlay.project ----------------------------------------------------------------------------------
def _same(pose, params, **kw):
    got = capi.overlay_project(pose, params)
    want = overlay.project(pose, **kw)
    assert got == (list(want[0]), want[1]), (np.asarray(pose).tolist(), got, want)
    return got[1]


def test_host_project_equals_restatement_on_oracle_poses(O, prm, template):
    drawn = 0
    for i in range(8):
        res = O.process_frame(synth.frame(i), prm, template)["result"]
        for k in range(min(res.n_clusters, capi.CD_MAX_CLUSTERS_PER_FRAME)):
            pose = np.array(res.clusters[k].pose)
            drawn += _same(pose, None)
            E = np.eye(4)
            E[:3, 3] = (0.015, -0.001, 0.002)
            drawn += _same(pose, capi.overlay_params(E=E, dims=(0.2, 0.075, 0.1)), E=E, dims=(0.2, 0.075, 0.1))
    assert drawn >= 16   # (every frame has at least one cluster, in front of the camera)


def test_host_project_equals_restatement_on_random_poses():
    from conftest import rot_xyz
    rng = np.random.default_rng(20190409)
    kinds = {0: 0, 1: 0}
    for i in range(400):
        T = np.eye(4)
        T[:3, :3] = rot_xyz(*rng.uniform(-np.pi, np.pi, 3))
        mode = i % 8
        if mode < 4:      # in view, roughly
            T[:3, 3] = rng.uniform((-0.4, -0.3, 0.2), (0.4, 0.3, 1.5))
        elif mode == 4:   # behind the camera
            T[:3, 3] = rng.uniform((-0.4, -0.3, -1.5), (0.4, 0.3, 0.05))
        elif mode == 5:   # far off-screen: around the 8192 bound and beyond
            T[:3, 3] = (rng.uniform(-40.0, 40.0), rng.uniform(-40.0, 40.0), rng.uniform(0.2, 2.0))
        elif mode == 6:   # a NaN or an infinity somewhere in the pose
            T[:3, 3] = (0.0, 0.0, 0.6)
            T[rng.integers(0, 3), rng.integers(0, 4)] = (np.nan, np.inf, -np.inf)[i % 3]
        else:             # large values and a scaled rotation
            T[:3, :3] *= rng.uniform(0.0, 1e6)
            T[:3, 3] = rng.uniform(-1e3, 1e3, 3)
        kinds[_same(T, None)] += 1
    assert kinds[0] >= 100 and kinds[1] >= 100, kinds


def test_host_project_checks_its_parameters():
    lib = capi.load_library()
    pose = np.eye(4)
    dp = C.POINTER(C.c_double)
    box = capi.CdOverlayBox()
    assert lib.cd_overlay_project(None, None, C.byref(box)) == capi.CD_ERR_INVALID_ARG
    assert lib.cd_overlay_project(pose.ctypes.data_as(dp), None, None) == capi.CD_ERR_INVALID_ARG
    for field, idx in (("P", 3), ("E", 7), ("dims", 1)):
        for v in (np.nan, np.inf):
            o = capi.default_overlay_params()
            getattr(o, field)[idx] = v
            assert lib.cd_overlay_project(pose.ctypes.data_as(dp), C.byref(o), C.byref(box)) == capi.CD_ERR_INVALID_ARG


# ---- the ctypes mirror ------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_of_the_overlay_structs():
    lib = capi.load_library()
    assert lib.cd_abi_version() == capi.CD_ABI_VERSION == 4
    assert lib.cd_struct_size(7) == C.sizeof(capi.CdOverlayParams) == 280
    assert lib.cd_struct_size(8) == C.sizeof(capi.CdOverlayBox) == 80
    assert lib.cd_struct_size(9) == -1
    for name in ("cd_default_overlay_params", "cd_overlay_project", "cd_draw_boxes_batch", "cd_draw_boxes_batch_device",
                 "cd_draw_last_results", "cd_draw_last_results_device"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    p = capi.CdOverlayParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    lib.cd_default_overlay_params(C.byref(p))
    assert bytes(p) == bytes(capi.default_overlay_params())
    assert list(p.P) == list(overlay.DEFAULT_P) and list(p.E) == list(overlay.DEFAULT_E) and list(p.dims) == [0.2, 0.1, 0.03]
    assert p.thickness == 2 and tuple(p.rgb) == (0, 255, 0)
    cam = capi.default_depth_camera()
    assert (p.P[0], p.P[5], p.P[2], p.P[6]) == (cam.fx, cam.fy, cam.cx, cam.cy)
